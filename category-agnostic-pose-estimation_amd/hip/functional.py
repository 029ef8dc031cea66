"""Autograd plumbing around the HIP kernels.

Each `torch.autograd.Function` here is glue: forward and backward only *launch* kernels of
libcape_hip.so (through `ops`) and keep the tensors backward needs.  No arithmetic of the hot path is
done by torch ops in this file.
"""
import contextlib
import ctypes
import os

import torch

from . import lib, ops


class Runtime:
    """Per-process runtime state shared by the Functions: dropout RNG state on device, and the
    weight-gradient sink: when parameters own gradient-arena views (runtime/arena.py) the wgrad kernels
    accumulate straight into them (GEMM epilogue `C += ...` / atomics) instead of materialising a tensor that
    autograd would add afterwards, and they run on a side stream so that they fill the idle CUs of the
    data-gradient chain's kernel tails.  `on_param_grad` callbacks let the data-parallel layer launch a
    bucket's all-reduce as soon as its gradients have been enqueued."""
    rng = None
    direct_grad = False
    use_side_stream = os.environ.get("CAPE_SIDE_STREAM", "1") == "1"
    side = None
    on_param_grad = []
    capture_keep = None          # list while a hipGraph capture is in progress (runtime/graph_step.py)

    pending = []                 # tensors read by enqueued side-stream kernels: kept alive until join()
    side_dirty = False           # work has been forked onto the side stream since the last join

    # Weight gradients are not launched where the backward pass produces them: nothing waits for one until the optimizer
    # step, so their GEMM descriptors are queued (per tile class) and submitted `wgrad_group` at a time as ONE grouped launch
    # (csrc/gemm_group.hip) -- and whatever is left when the autograd engine finishes the pass.  Round 2 paid 199 launches,
    # 24-64 k-splits each to fill the chip alone, for what is now ~15 launches of 4-8 k-splits.  Two products of one group never
    # write overlapping bytes (items with split_k == 1 add into C without atomics): such a product launches the queued class first.
    defer_wgrad = os.environ.get("CAPE_DEFER_WGRAD", "1") == "1"
    wgrad_group = int(os.environ.get("CAPE_WGRAD_GROUP", "12"))
    wq = {}                      # (tile, b_mode, precision) -> [(desc, keep, shape, destination byte ranges)]
    wq_total = 0
    wq_notify = []               # parameters whose notification (data-parallel bucket bookkeeping) waits for the queued products
    _final_cb = False            # the end-of-pass flush is registered with the running backward pass

    @classmethod
    def side_stream(cls):
        if cls.side is None:
            cls.side = torch.cuda.Stream()
            cls.side_raw = cls.side.cuda_stream
        return cls.side

    @classmethod
    def join(cls):
        """Make the current stream wait for all enqueued side-stream work (call before the optimizer step)."""
        cls.flush_wgrads()
        if cls.side is not None and cls.side_dirty:     # (nothing forked since the last join: no event to wait for -- a capture that
            cls.side_dirty = False                      #  only holds the optimizer step must not touch the un-captured side stream)
            lib.call("cape_stream_join", ctypes.c_void_p(ops.raw_current_stream()), ctypes.c_void_p(cls.side_raw))
            if cls.capture_keep is None:
                cls.pending.clear()

    @classmethod
    def notify(cls, *params):
        if cls.wq_total or cls.wq_notify:               # behind queued products: the callbacks run when those have been launched
            cls.wq_notify.extend(p for p in params if p is not None)
            return
        for cb in cls.on_param_grad:
            for p in params:
                if p is not None:
                    cb(p)

    @classmethod
    def enqueue_wgrad(cls, desc, keep):
        M, N, K, b_mode = desc.M, desc.N, desc.K, desc.b_mode
        key = (ops.group_tile(M, N, K), b_mode, desc.precision)
        dst = [(desc.C, desc.C + 4 * ((M - 1) * desc.ldc + N))]
        if desc.colsum_out:
            dst.append((desc.colsum_out, desc.colsum_out + 4 * M))
        items = cls.wq.setdefault(key, [])
        if any(lo < e and s < hi for it in items for s, e in it[3] for lo, hi in dst):
            cls._launch_class(key)                      # (the same weight again, e.g. a layer applied twice): its group goes first
        cls.wq[key].append((desc, keep, (M, N, K, 1, b_mode), dst))
        cls.wq_total += 1
        if not cls._final_cb:
            try:                                        # whatever is still queued when this backward pass ends goes then
                torch.autograd.Variable._execution_engine.queue_callback(cls.flush_wgrads)
                cls._final_cb = True
            except RuntimeError:                        # not inside a backward pass (a Function driven by hand): no deferral
                cls.flush_wgrads()
                return
        if cls.wq_total >= cls.wgrad_group or len(cls.wq[key]) >= lib.GEMM_GROUP_MAX:
            cls._flush()

    @classmethod
    def _launch_class(cls, key):
        items = cls.wq.get(key)
        if not items:
            return
        cls.wq[key] = []
        cls.wq_total -= len(items)
        tile = key[0]
        shapes = [it[2] for it in items]
        for it, sk in zip(items, ops.plan_group_splits([sh[:3] for sh in shapes], tile)):
            it[0].split_k = sk
        with _Side([t for it in items for t in it[1]]):
            for i in range(0, len(items), lib.GEMM_GROUP_MAX):
                ops.gemm_group([it[0] for it in items[i:i + lib.GEMM_GROUP_MAX]], shapes[i:i + lib.GEMM_GROUP_MAX], tile)

    @classmethod
    def flush_wgrads(cls):
        """Launch every queued weight-gradient product (one grouped launch per tile class) and run the notifications
        that waited for them.  The next queued product registers a new end-of-pass flush (also after a pass that raised)."""
        cls._final_cb = False
        cls._flush()

    @classmethod
    def _flush(cls):
        for key in list(cls.wq):
            cls._launch_class(key)
        if cls.wq_notify:
            ps, cls.wq_notify = cls.wq_notify, []
            for cb in cls.on_param_grad:
                for p in ps:
                    cb(p)

    @classmethod
    def get_rng(cls, device):
        if cls.rng is None:
            cls.rng = ops.RngState(0x5EED, device)
        return cls.rng

    @classmethod
    def seed(cls, seed, device):
        cls.rng = ops.RngState(int(seed), device)


def capturing():
    """True while the current stream is being captured into a hipGraph: host decisions that would need a
    device->host sync take their conservative branch, and cross-stream lifetimes are handled by keeping tensors alive."""
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


def _c(t):
    return t if (t is None or t.is_contiguous()) else t.contiguous()


class _Side:
    """Context of side-stream work: kernels launched inside go to the side stream, ordered after the current stream's work so far (one C
    call at the block's first launch: event record + wait; no framework stream switch); the tensors are kept alive until the next
    join -- the caching allocator may otherwise hand their blocks to a later main-stream kernel while the side kernel still reads
    them.  Blocks nest (a group launched from inside a node's block)."""

    def __init__(self, tensors):
        self.tensors = [t for t in tensors if t is not None]

    def __enter__(self):
        self.on, self.forked, self.prev = Runtime.use_side_stream, False, ops._side[0]
        if self.on:
            Runtime.side_stream()
            ops._side[0] = self._raw
        return self

    def _raw(self):
        if not self.forked:                             # (a block whose products are all queued launches nothing: no fork)
            self.forked = True
            lib.call("cape_stream_fork", ctypes.c_void_p(ops.raw_current_stream()), ctypes.c_void_p(Runtime.side_raw))
            Runtime.side_dirty = True
        return Runtime.side_raw

    def __exit__(self, *a):
        if not self.on:
            return False
        ops._side[0] = self.prev
        (Runtime.capture_keep if Runtime.capture_keep is not None else Runtime.pending).extend(self.tensors)
        if len(Runtime.pending) > 8192:                 # a caller that never joins (backward without an optimizer step)
            Runtime.join()
        return False


def _groupable(d):
    """A weight-gradient product that cape_gemm_group_f32 takes: C += A^T B (dense or im2col B) with at most the fused bias sums,
    on the vector path of the tile body (16-byte aligned operands and rows)."""
    return (d.a_mode == 1 and d.accumulate and d.b_mode in (1, 3) and d.batch == 0 and d.mask_src is None and d.bias is None
            and d.A % 16 == 0 and d.B % 16 == 0 and d.lda % 4 == 0 and d.M % 4 == 0 and d.M >= 4 and d.N % 4 == 0 and d.N >= 4
            and (d.b_mode == 3 or d.ldb % 4 == 0) and max(d.lda, d.ldb, d.ldc) < (1 << 31))


_NO_SIDE = contextlib.nullcontext()


class _ParamGrads:
    """Where the parameter gradients of one node backward go.  `bufs[i]` receives the gradient of refs[i] (None when it needs none):
      * direct -- EVERY parameter the node must differentiate owns a gradient-arena view (runtime/arena.py): the kernels accumulate
        into those views (inside side(): on the side stream; wgrad products issued through gemm() join the deferred groups,
        Runtime.defer_wgrad); result() notifies each parameter once and hands autograd Nones;
      * otherwise fresh zero tensors (the parameter's layout: a channels_last conv weight stays channels_last), written on the main
        stream and returned by result().  All or nothing: a side-stream kernel never writes a tensor that autograd reads.
    needs: per ref, whether it is differentiated (default: every ref that is not None)."""

    def __init__(self, refs, needs=None):
        self.refs = refs
        self.needs = [r is not None and (needs is None or bool(needs[i])) for i, r in enumerate(refs)]
        views = [self._view(r) if n else None for r, n in zip(refs, self.needs)]
        self.direct = any(self.needs) and all(v is not None for v, n in zip(views, self.needs) if n)
        self.bufs = views if self.direct else [torch.zeros_like(r) if n else None for r, n in zip(refs, self.needs)]

    @staticmethod
    def _view(p):
        """Gradient-arena view of parameter `p` (or of the parameter `p` is a plain view of), else None."""
        if not Runtime.direct_grad or not p.requires_grad:
            return None
        if isinstance(p, torch.nn.Parameter):
            return p.grad
        base = p._base
        if isinstance(base, torch.nn.Parameter) and base.grad is not None and base.requires_grad:
            off = p.storage_offset() - base.storage_offset() + base.grad.storage_offset()
            return torch.as_strided(base.grad, p.shape, p.stride(), off)
        return None

    def side(self, *tensors):
        """Context of the node's side-stream work (may be entered more than once); a no-op unless direct.  `tensors`: what it reads."""
        return _Side(tensors) if self.direct else _NO_SIDE

    def gemm(self, *args, **kw):
        """A weight-gradient product (ops.gemm arguments): queued for a grouped launch when direct and deferring, else launched."""
        d, keep = ops.gemm_desc(*args, **kw)
        if self.direct and Runtime.defer_wgrad and _groupable(d):
            Runtime.enqueue_wgrad(d, keep)
        else:
            ops.launch_gemm(d)

    def result(self):
        """The node's return values for refs: the fresh gradients, or Nones after one notification per differentiated parameter."""
        if not self.direct:
            return tuple(self.bufs)
        Runtime.notify(*[r if isinstance(r, torch.nn.Parameter) else r._base for r, n in zip(self.refs, self.needs) if n])
        return (None,) * len(self.refs)


class _Slot:
    """Gradient slot of a tensor with several consumers (see `fanout`): the first consumer whose backward produces an exclusively
    owned data gradient leaves its buffer here; later consumers ADD theirs into it (GEMM `C += ...` epilogue) instead of writing
    a buffer of their own that a summation pass then reads again."""
    __slots__ = ("buf",)

    def __init__(self):
        self.buf = None


_SLOTS = os.environ.get("CAPE_GRAD_SLOTS", "1") == "1"


def _slot_of(x):
    return getattr(x, "_cape_slot", None) if _SLOTS else None


def _grad_target(slot, shape, device):
    """(buffer viewed as `shape`, accumulate?) for a data gradient of `shape` (contiguous)."""
    if slot is not None and slot.buf is not None:
        b = slot.buf
        if b.is_contiguous() and b.numel() == int(torch.Size(shape).numel()) and b.device == device:
            return b.view(shape), True
    buf = torch.empty(shape, dtype=torch.float32, device=device)
    if slot is not None and slot.buf is None:
        slot.buf = buf
    return buf, False


def _slot_offer(slot, buf):
    """A non-GEMM producer (LayerNorm backward) offers its freshly written, exclusively owned gradient buffer."""
    if slot is not None and slot.buf is None and buf is not None and buf.is_contiguous():
        slot.buf = buf


# ------------------------------------------------------------------------------------------------
# Linear (+bias, +relu, +dropout, +residual) -- F.linear and its autograd
# ------------------------------------------------------------------------------------------------
class LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, residual, relu, dropout_p, rng_stream):
        K = x.shape[-1]
        N = weight.shape[0]
        assert weight.shape[1] == K and weight.stride(1) == 1
        x2 = _c(x).view(-1, K)
        M = x2.shape[0]
        res2 = _c(residual).view(-1, N) if residual is not None else None
        y = torch.empty(M, N, dtype=torch.float32, device=x.device)
        rng = Runtime.get_rng(x.device) if dropout_p > 0 else None
        ops.gemm(x2, weight, y, M, N, K, ldb=weight.stride(0), bias=bias, residual=res2, relu=relu, dropout_p=dropout_p,
                 rng=rng, rng_stream=rng_stream)
        ctx.save_for_backward(x2, weight, y if (relu or dropout_p > 0) else None)
        ctx.w_ref, ctx.b_ref = weight, bias
        ctx.slot = _slot_of(x)
        ctx.meta = (relu, dropout_p, bias is not None, residual is not None, x.shape, M, N, K)
        return y.view(*x.shape[:-1], N)

    @staticmethod
    def backward(ctx, dy):
        x2, weight, y = ctx.saved_tensors
        relu, p, has_bias, has_res, xshape, M, N, K = ctx.meta
        dy2 = _c(dy).view(M, N)
        dpre = dy2
        if relu or p > 0:
            assert relu, "dropout epilogue is only used together with relu"
            dpre = ops.relu_drop_bwd(dy2, y, 1.0 / (1.0 - p) if p > 0 else 1.0)
        dx = None
        if ctx.needs_input_grad[0]:
            dx, acc = _grad_target(ctx.slot, (M, K), dy.device)
            ops.gemm(dpre, weight, dx, M, K, N, a_mode=0, b_mode=1, ldb=weight.stride(0), accumulate=acc)
            dx = dx.view(xshape)
        pg = _ParamGrads((ctx.w_ref, ctx.b_ref), ctx.needs_input_grad[1:3])
        dw, db = pg.bufs
        with pg.side(dpre, x2):
            if dw is not None:                          # the bias sums ride in the wgrad
                pg.gemm(dpre, x2, dw, N, K, M, a_mode=1, b_mode=1, lda=N, ldb=K, ldc=dw.stride(0), accumulate=True,
                        split_k=ops.pick_split_k(N, K, M), colsum_out=db)
            elif db is not None:
                ops.colsum(dpre, M, N, db)
        dres = dy if (has_res and ctx.needs_input_grad[3]) else None
        return (dx,) + pg.result() + (dres, None, None, None)


def linear(x, weight, bias=None, residual=None, relu=False, dropout_p=0.0, rng_stream=0):
    return LinearFn.apply(x, weight, bias, residual, relu, float(dropout_p), int(rng_stream))


class FFNFn(torch.autograd.Function):
    """y = (dropout(relu(x W1^T + b1))) W2^T + b2 -- the transformer feed-forward pair as one node, so that the backward
    can let the dgrad of the second linear emit the pre-activation gradient of the first directly (GEMM epilogue gated by
    the saved hidden activation) instead of running a separate relu/dropout-backward pass over the (rows x 1024) tensor."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, dropout_p, rng_stream):
        K, Hd, N = x.shape[-1], w1.shape[0], w2.shape[0]
        x2 = _c(x).view(-1, K)
        M = x2.shape[0]
        rng = Runtime.get_rng(x.device) if dropout_p > 0 else None
        h = torch.empty(M, Hd, dtype=torch.float32, device=x.device)
        ops.gemm(x2, w1, h, M, Hd, K, ldb=w1.stride(0), bias=b1, relu=True, dropout_p=dropout_p, rng=rng, rng_stream=rng_stream)
        y = torch.empty(M, N, dtype=torch.float32, device=x.device)
        ops.gemm(h, w2, y, M, N, Hd, ldb=w2.stride(0), bias=b2)
        ctx.save_for_backward(x2, w1, w2, h)
        ctx.refs = (w1, b1, w2, b2)
        ctx.slot = _slot_of(x)
        ctx.meta = (dropout_p, x.shape, M, K, Hd, N)
        return y.view(*x.shape[:-1], N)

    @staticmethod
    def backward(ctx, dy):
        x2, w1, w2, h = ctx.saved_tensors
        p, xshape, M, K, Hd, N = ctx.meta
        dy2 = _c(dy).view(M, N)
        # d(pre-activation of linear1) = (dy W2) gated by the saved hidden activation
        dpre = torch.empty(M, Hd, dtype=torch.float32, device=dy.device)
        ops.gemm(dy2, w2, dpre, M, Hd, N, a_mode=0, b_mode=1, ldb=w2.stride(0), mask_src=h, mask_scale=1.0 / (1.0 - p) if p > 0 else 1.0)
        dx = None
        if ctx.needs_input_grad[0]:
            dx, acc = _grad_target(ctx.slot, (M, K), dy.device)
            ops.gemm(dpre, w1, dx, M, K, Hd, a_mode=0, b_mode=1, ldb=w1.stride(0), accumulate=acc)
            dx = dx.view(xshape)
        pg = _ParamGrads(ctx.refs)
        dw1, db1, dw2, db2 = pg.bufs
        with pg.side(dy2, dpre, h, x2):
            pg.gemm(dy2, h, dw2, N, Hd, M, a_mode=1, b_mode=1, lda=N, ldb=Hd, ldc=dw2.stride(0), accumulate=True,
                    split_k=ops.pick_split_k(N, Hd, M), colsum_out=db2)
            pg.gemm(dpre, x2, dw1, Hd, K, M, a_mode=1, b_mode=1, lda=Hd, ldb=K, ldc=dw1.stride(0), accumulate=True,
                    split_k=ops.pick_split_k(Hd, K, M), colsum_out=db1)
        return (dx,) + pg.result() + (None, None)


_NO_FFN_FUSE = os.environ.get("CAPE_NO_FFN_FUSE") is not None
# CAPE_DETERMINISTIC=1: no atomic k-split in the forward pass (convolution forward), so activations are bitwise reproducible
# run to run.  The backward k-splits stay: the backward pass is linear in dY for fixed activations, their arrival-order
# rounding (~1e-6 of the gradient) is not amplified.  Measured (tools/lab/determinism.py, profiles/
# r02_determinism.txt): this model turns a 1.2e-7 relative perturbation of the input image into a 3e-3..7e-3 relative change
# of the gradient (discontinuous pieces: bilinear-sampling cell boundaries, L1 signs, ReLU gates), and the forward
# k-splits' arrival order does the same -- comparable to the bf16x3 / fp32 difference, invisible to training, but too
# large for tests that compare two executions of the same mathematics at 2e-4.
_DETERMINISTIC = os.environ.get("CAPE_DETERMINISTIC", "0") == "1"


def ffn(x, w1, b1, w2, b2, dropout_p=0.0, rng_stream=0):
    """linear2(dropout(relu(linear1(x)))) with both biases (deformable_transformer.py:95,99-100; deformable_transformer_v2.py:
    314-318; nn.TransformerEncoderLayer's feed-forward in geometric_support_encoder.py)."""
    if _NO_FFN_FUSE:          # tuning switch: two separate linear nodes (relu/dropout backward as its own pass)
        return linear(linear(x, w1, b1, relu=True, dropout_p=dropout_p, rng_stream=rng_stream), w2, b2)
    return FFNFn.apply(x, w1, b1, w2, b2, float(dropout_p), int(rng_stream))


def _adjacent(a, b):
    """b starts where a ends, in the same storage (both dense, row-major)."""
    return (a.is_contiguous() and b.is_contiguous() and a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()
            and b.data_ptr() == a.data_ptr() + a.numel() * a.element_size())


class LinearCat2Fn(torch.autograd.Function):
    """[x W1^T + b1 | x W2^T + b2]  (sampling offsets | attention logits of MSDeformAttn)."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2):
        K = x.shape[-1]
        N1, N2 = w1.shape[0], w2.shape[0]
        x2 = _c(x).view(-1, K)
        M = x2.shape[0]
        y = torch.empty(M, N1 + N2, dtype=torch.float32, device=x.device)
        # in the flat arenas the two weights (and the two biases) sit back to back (runtime/arena._colocate): one launch
        adjacent = _adjacent(w1, w2) and _adjacent(b1, b2)
        if adjacent:
            ops.gemm(x2, torch.as_strided(w1, (N1 + N2, K), (K, 1)), y, M, N1 + N2, K, bias=torch.as_strided(b1, (N1 + N2,), (1,)))
        else:
            ops.gemm(x2, w1, y, M, N1, K, bias=b1, ldc=N1 + N2)
            ops.gemm(x2, w2, y[:, N1:], M, N2, K, bias=b2, ldc=N1 + N2)
        ctx.save_for_backward(x2, w1, w2)
        ctx.refs = (w1, b1, w2, b2)
        ctx.meta = (x.shape, M, N1, N2, K, adjacent)
        return y.view(*x.shape[:-1], N1 + N2)

    @staticmethod
    def backward(ctx, dy):
        x2, w1, w2 = ctx.saved_tensors
        xshape, M, N1, N2, K, adjacent = ctx.meta
        NT = N1 + N2
        dy2 = _c(dy).view(M, NT)
        dev = dy.device
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty(M, K, dtype=torch.float32, device=dev)
            ops.gemm(dy2, w1, dx, M, K, N1, a_mode=0, b_mode=1, lda=NT)
            ops.gemm(dy2[:, N1:], w2, dx, M, K, N2, a_mode=0, b_mode=1, lda=NT, accumulate=True)
            dx = dx.view(xshape)
        pg = _ParamGrads(ctx.refs)
        dw1, db1, dw2, db2 = pg.bufs
        with pg.side(dy2, x2):
            if adjacent and _adjacent(dw1, dw2) and _adjacent(db1, db2):      # the gradients mirror the layout: one product
                pg.gemm(dy2, x2, torch.as_strided(dw1, (NT, K), (K, 1)), NT, K, M, a_mode=1, b_mode=1, lda=NT, accumulate=True,
                        split_k=ops.pick_split_k(NT, K, M), colsum_out=torch.as_strided(db1, (NT,), (1,)))
            else:
                for dw, db, lo, n in ((dw1, db1, 0, N1), (dw2, db2, N1, N2)):
                    pg.gemm(dy2[:, lo:], x2, dw, n, K, M, a_mode=1, b_mode=1, lda=NT, accumulate=True, split_k=ops.pick_split_k(n, K, M),
                            colsum_out=db)
        return (dx,) + pg.result()


def linear_cat2(x, w1, b1, w2, b2):
    return LinearCat2Fn.apply(x, w1, b1, w2, b2)


# ------------------------------------------------------------------------------------------------
# Convolution (NHWC, channels_last weights) + folded FrozenBN / bias + ReLU + residual
# ------------------------------------------------------------------------------------------------
def _w_phys(weight):
    """(O, C, KH, KW) channels_last parameter -> its physical (O, KH, KW, C) contiguous view."""
    wp = weight.permute(0, 2, 3, 1)
    assert wp.is_contiguous(), "conv weights must be stored channels_last"
    return wp


def _conv_stage_fwd(x, weight, scale, shift, residual, stride, pad, relu, allow_split, dil=1):
    """One convolution stage, y = act(conv(x) * scale + shift + residual), as a plain function: -> (y, meta, saved).  `meta` is
    the non-tensor record and `saved` the tensors `_conv_stage_bwd` needs; the calling autograd node hands `saved` to its own
    save_for_backward (x is (N, H, W, C) NHWC).  `dil`: the convolution's dilation (torch's `dilation=`), kept in `meta` beside the
    11-tuple geometry."""
    x = _c(x)
    N, H, W, C = x.shape
    O, C2, KH, KW = weight.shape
    assert C2 == C
    wp = _w_phys(weight)
    OH, OW = (H + 2 * pad - dil * (KH - 1) - 1) // stride + 1, (W + 2 * pad - dil * (KW - 1) - 1) // stride + 1
    M, K = N * OH * OW, KH * KW * C
    y = torch.empty(N, OH, OW, O, dtype=torch.float32, device=x.device)
    res = _c(residual) if residual is not None else None
    geom = (N, H, W, C, KH, KW, stride, pad, OH, OW, O)
    dense = KH == 1 and KW == 1 and stride == 1 and pad == 0
    # few output tiles over a deep contraction (the 3x3/s2 input_proj conv on C5: 512 x 256 x 18432 = 32 tiles; the 3x3
    # convolutions of layer4: 2048 x 512 x 4608 = 256 tiles of 144 k-tiles each): split K over blocks (atomic partial sums,
    # the bias rides with the first split) and apply FrozenBN / ReLU / shortcut in a separate in-place pass.  Training
    # only: the atomic k-split sums in arrival order, and inference keeps run-to-run bitwise reproducibility (the
    # replayed decode graphs are tested bit-for-bit against the eager loop).
    # (`allow_split` = grad mode at the call site: autograd runs Function.forward itself with grad mode off)
    sk = ops.pick_split_k(M, O, K) if (allow_split and not _DETERMINISTIC) else 1
    plain = scale is None and res is None and not relu
    sk = sk if (sk >= 8 or (sk >= 4 and not plain)) else 1
    if sk > 1:
        y.zero_()
        kw = dict(bias=shift if plain else None, split_k=sk, accumulate=True)
    else:
        kw = dict(scale=scale, bias=shift, residual=res, relu=relu)
    if dense:
        ops.gemm(x, wp, y, M, O, K, **kw)
    else:
        ops.gemm(x, wp, y, M, O, K, a_mode=2, b_mode=0, conv=geom, conv_dil=dil, **kw)
    if sk > 1 and not plain:
        ops.affine_act_(y, scale, shift, res, relu)
    return y, (geom, dense, relu, residual is not None, dil), (x, weight, scale, y if relu else None)


def _conv_stage_bwd(meta, saved, dy, w_ref, shift_ref=None, *, need_x, need_w=False, need_shift=False, need_res=False, acc_dx=None):
    """Backward of one `_conv_stage_fwd` call: -> (dx, dw, dshift, dres), each None unless its need_* is set.  `w_ref` /
    `shift_ref`: the parameters as the node received them (`_ParamGrads` finds their gradient-arena views).  `acc_dx`: a
    gradient of the same input that already exists (the bottleneck's shortcut branch) -- the data gradient is added into it by
    the accumulate epilogue instead of a separate summation pass, and it is returned as dx."""
    x, weight, scale, y = saved
    geom, dense, relu, has_res, dil = meta
    N, H, W, C, KH, KW, stride, pad, OH, OW, O = geom
    dy = _c(dy)
    M, K = N * OH * OW, KH * KW * C
    want_res = has_res and need_res
    if relu or scale is not None or want_res:
        dpre, dres = ops.bn_relu_bwd(dy, y if relu else dy, scale, relu, want_res) if scale is not None else \
            _relu_bwd_noscale(dy, y, relu, want_res)
    else:
        dpre, dres = dy, None
    wp = _w_phys(weight)
    dx = None
    if need_x:
        dx = acc_dx if acc_dx is not None else torch.empty(N, H, W, C, dtype=torch.float32, device=dy.device)
        if dense:
            ops.gemm(dpre, wp, dx, M, C, O, a_mode=0, b_mode=1, accumulate=acc_dx is not None)
        elif dil == 1 and _dgrad_stride2_ok(geom):       # (the parity classes are worked out for undilated taps)
            _dgrad_stride2(dpre, wp, geom, dx, acc_dx)
        else:
            sk = ops.pick_split_k(N * H * W, C, KH * KW * O)
            sk = sk if sk >= 4 else 1
            if sk > 1 and acc_dx is None:
                dx.zero_()
            ops.gemm(dpre, wp, dx, N * H * W, C, KH * KW * O, a_mode=3, b_mode=2, conv=geom, conv_dil=dil, split_k=sk,
                     accumulate=sk > 1 or acc_dx is not None)
    # the weight gradient is computed in the physical (O, KH, KW, C) layout of the channels_last weight (and of its gradient)
    pg = _ParamGrads((w_ref, shift_ref), (need_w, need_shift))
    dw, dshift = pg.bufs
    src_s = None
    if dshift is not None:
        src_s = dpre if scale is None else (dres if dres is not None else _mask_only(dy, y, relu))
    with pg.side(dpre, x, src_s):
        fuse_s = src_s is dpre and dw is not None   # the bias sums ride in the wgrad
        if dw is not None:
            kw = dict(a_mode=1, lda=O, accumulate=True, colsum_out=dshift if fuse_s else None)
            if dense:
                pg.gemm(dpre, x, _w_phys(dw), O, C, M, b_mode=1, ldb=C, split_k=ops.pick_split_k(O, C, M), **kw)
            else:
                pg.gemm(dpre, x, _w_phys(dw), O, K, M, b_mode=3, conv=geom, conv_dil=dil, split_k=ops.pick_split_k(O, K, M), **kw)
        if dshift is not None and not fuse_s:
            ops.colsum(src_s, M, O, dshift)
    return (dx,) + pg.result() + (dres,)


class ConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, scale, shift, residual, stride, pad, relu, allow_split=False, dilation=1):
        y, ctx.meta, saved = _conv_stage_fwd(x, weight, scale, shift, residual, stride, pad, relu, allow_split, dilation)
        ctx.save_for_backward(*saved)
        ctx.w_ref, ctx.shift_ref = weight, shift
        return y

    @staticmethod
    def backward(ctx, dy):
        need_x, need_w, _, need_shift, need_res = ctx.needs_input_grad[:5]
        dx, dw, dshift, dres = _conv_stage_bwd(ctx.meta, ctx.saved_tensors, dy, ctx.w_ref, ctx.shift_ref, need_x=need_x,
                                               need_w=need_w, need_shift=need_shift, need_res=need_res)
        return dx, dw, None, dshift, dres, None, None, None, None, None


_DGRAD_S2 = os.environ.get("CAPE_DGRAD_S2_CLASSES", "1") == "1"


def _dgrad_stride2_ok(geom):
    N, H, W, C, KH, KW, stride, pad, OH, OW, O = geom
    return (_DGRAD_S2 and stride == 2 and H % 2 == 0 and W % 2 == 0 and OH * 2 == H and OW * 2 == W and O % 32 == 0 and C % 4 == 0
            and (KH, KW, pad) in ((3, 3, 1), (1, 1, 0)))


def _dgrad_stride2(dpre, wp, geom, dx, acc_dx):
    """Data gradient of a stride-2 convolution (3x3 / pad 1, or 1x1) by input-parity classes.  As one gather launch over the
    full-resolution grid 3 of 4 (pixel, tap) pairs multiply structural zeros (a tap reaches a pixel only when the parities fit).
    The pixels (2y' + py, 2x' + px) of one class see a fixed subset of the taps and their gradient is a STRIDE-1 data gradient on
    the half-resolution grid: rows py = 1 use taps kh in {0, 2} with padding 1, rows py = 0 the tap kh = 1 with padding 0 (same
    for columns): 4 + 2 + 2 + 1 = 9 taps over 4 pixels instead of 36.  The four compact results go back onto the grid (and onto a
    gradient that already exists there: the shortcut branch's) in one pass.  1x1 / stride 2: only the (even, even) class is
    non-zero and it is a dense product."""
    N, H, W, C, KH, KW, stride, pad, OH, OW, O = geom
    H2, W2 = H // 2, W // 2
    Mc = N * H2 * W2
    dev = dpre.device
    classes = [None] * 4
    if KH == 1:
        c00 = torch.empty(N, H2, W2, C, dtype=torch.float32, device=dev)
        ops.gemm(dpre, wp, c00, Mc, C, O, a_mode=0, b_mode=1)
        classes[0] = c00
    else:
        for py in (0, 1):
            for px in (0, 1):
                kh_n, kw_n = (2 if py else 1), (2 if px else 1)
                sub_geom = (N, H2, W2, C, kh_n, kw_n, 1, (1 if py else 0), OH, OW, O)
                sub = ((1 if px else 0), KH, KW, (0 if py else 1), 2, (0 if px else 1), 2)
                K = kh_n * kw_n * O
                buf = torch.empty(N, H2, W2, C, dtype=torch.float32, device=dev)
                sk = ops.pick_split_k(Mc, C, K)
                sk = sk if sk >= 4 else 1
                if sk > 1:
                    buf.zero_()
                ops.gemm(dpre, wp, buf, Mc, C, K, a_mode=3, b_mode=2, conv=sub_geom, conv_sub=sub, split_k=sk, accumulate=sk > 1)
                classes[py * 2 + px] = buf
    ops.interleave2x2(classes, acc_dx, dx)


def _relu_bwd_noscale(dy, y, relu, want_res):
    if not relu:
        return dy, (dy if want_res else None)
    d = ops.relu_drop_bwd(dy, y, 1.0)
    return d, (d if want_res else None)


def _mask_only(dy, y, relu):
    return ops.relu_drop_bwd(dy, y, 1.0) if relu else dy


class BottleneckFn(torch.autograd.Function):
    """torchvision Bottleneck v1.5 with FrozenBatchNorm2d (reference backbone.py:20-57 over torchvision.models.resnet50) as ONE
    autograd node: conv1-bn-relu, conv2(3x3, stride, dilation; padding = dilation)-bn-relu, [downsample conv-bn], conv3-bn + shortcut + relu.  The backward
    runs the four conv stages in order and lets conv1's data gradient accumulate into the shortcut's gradient (the block
    input has two consumers; as separate nodes their gradients cost a summation pass over the largest tensors of the trunk),
    and the host pays for one node instead of five."""

    @staticmethod
    def forward(ctx, x, w1, w2, w3, wd, s1, b1, s2, b2, s3, b3, sd, bd, stride, allow_split, dilation=1):
        o1, m1, t1 = _conv_stage_fwd(x, w1, s1, b1, None, 1, 0, True, allow_split)
        o2, m2, t2 = _conv_stage_fwd(o1, w2, s2, b2, None, stride, dilation, True, allow_split, dilation)
        idt, md, td = x, None, ()
        if wd is not None:
            idt, md, td = _conv_stage_fwd(x, wd, sd, bd, None, stride, 0, False, allow_split)
        y, m3, t3 = _conv_stage_fwd(o2, w3, s3, b3, idt, 1, 0, True, allow_split)
        # every tensor the four stages keep goes through the node's own save_for_backward: the block output `y` is among
        # them (conv3's ReLU mask), and an output held as a plain attribute of the context is a reference cycle through its
        # grad_fn that Python's collector cannot see -- round 2 leaked ~1.4 GiB of trunk activations per training step that way
        ctx.save_for_backward(*t1, *t2, *t3, *td)
        ctx.cuts = (len(t1), len(t1) + len(t2), len(t1) + len(t2) + len(t3))
        ctx.metas = (m1, m2, m3, md)
        ctx.w_refs = (w1, w2, w3, wd)
        return y

    @staticmethod
    def backward(ctx, dy):
        t, (a, b, c) = ctx.saved_tensors, ctx.cuts
        t1, t2, t3, td = t[:a], t[a:b], t[b:c], t[c:]
        m1, m2, m3, md = ctx.metas
        w1, w2, w3, wd = ctx.w_refs
        need_x, need_w1, need_w2, need_w3, need_wd = ctx.needs_input_grad[:5]
        d2, dw3, _, dres = _conv_stage_bwd(m3, t3, dy, w3, need_x=True, need_w=need_w3, need_res=need_x or wd is not None)
        d1, dw2, _, _ = _conv_stage_bwd(m2, t2, d2, w2, need_x=True, need_w=need_w2)
        dwd, dshort = None, (dres if need_x else None)       # the block input's gradient through the shortcut
        if wd is not None:
            dshort, dwd, _, _ = _conv_stage_bwd(md, td, dres, wd, need_x=need_x, need_w=need_wd)
        dx, dw1, _, _ = _conv_stage_bwd(m1, t1, d1, w1, need_x=need_x, need_w=need_w1, acc_dx=dshort)
        return (dx, dw1, dw2, dw3, dwd) + (None,) * 11


def bottleneck(x, w1, w2, w3, wd, bn1, bn2, bn3, bnd, stride, dilation=1):
    """bnK = (scale, shift) of the folded FrozenBatchNorm2d; wd / bnd = None without a projection shortcut.  `dilation`: of the
    3x3 stage, whose padding equals it (torchvision conv3x3); the three 1x1 stages do not change."""
    sd, bd = bnd if bnd is not None else (None, None)
    return BottleneckFn.apply(x, w1, w2, w3, wd, bn1[0], bn1[1], bn2[0], bn2[1], bn3[0], bn3[1], sd, bd, int(stride), torch.is_grad_enabled(),
                              int(dilation))


def conv_bn_act(x, weight, scale, shift, stride=1, pad=0, relu=False, residual=None, dilation=1):
    return ConvFn.apply(x, weight, scale, shift, residual, int(stride), int(pad), bool(relu), torch.is_grad_enabled(), int(dilation))


# ------------------------------------------------------------------------------------------------
# LayerNorm(x + dropout(y)) [+ pos]
# ------------------------------------------------------------------------------------------------
class AddLayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, gamma, beta, pos, dropout_p, rng_stream):
        x, y, pos = _c(x), _c(y), _c(pos)
        rng = Runtime.get_rng(x.device) if dropout_p > 0 else None
        out, mean, rstd, out_pos = ops.add_layernorm_fwd(x, y, gamma, beta, pos=pos, dropout_p=dropout_p, rng=rng,
                                                         rng_stream=rng_stream)
        ctx.save_for_backward(x, y, gamma, mean, rstd)
        ctx.refs = (gamma, beta)
        ctx.slot = _slot_of(x)
        ctx.meta = (dropout_p, rng_stream, pos is not None)
        ctx.set_materialize_grads(False)        # an unused output arrives as None, not as a zero-filled tensor
        if pos is None:
            return out
        return out, out_pos

    @staticmethod
    def backward(ctx, d_out, d_out_pos=None):
        x, y, gamma, mean, rstd = ctx.saved_tensors
        p, stream, has_pos = ctx.meta
        g_pos = d_out_pos                       # out_pos = out + pos: its gradient reaches `pos` unchanged
        if d_out is None and d_out_pos is None:
            return None, None, None, None, None, None, None
        if d_out is None:
            d_out, d_out_pos = d_out_pos, None
        d_out, d_out_pos = _c(d_out), _c(d_out_pos)
        pg = _ParamGrads(ctx.refs)
        rng = Runtime.get_rng(x.device) if p > 0 else None
        dx, dy = ops.add_layernorm_bwd(d_out, d_out_pos, x, y, gamma, mean, rstd, *pg.bufs, dropout_p=p, rng=rng,
                                       rng_stream=stream)
        if y is None or dy is not dx:               # (without dropout the kernel hands ONE buffer to x and y: not exclusively x's)
            _slot_offer(ctx.slot, dx)
        dpos = g_pos if (has_pos and ctx.needs_input_grad[4]) else None
        return (dx, (dy if y is not None else None)) + pg.result() + (dpos, None, None)


def add_layernorm(x, y, gamma, beta, pos=None, dropout_p=0.0, rng_stream=0):
    return AddLayerNormFn.apply(x, y, gamma, beta, pos, float(dropout_p), int(rng_stream))


class AddFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        return ops.add(_c(a), _c(b))

    @staticmethod
    def backward(ctx, g):
        return g, g


def add(a, b):
    return AddFn.apply(a, b)


class FanOutFn(torch.autograd.Function):
    """x -> k aliases of x for k consumers.  Autograd would sum the k incoming gradients of a multiply-used tensor with k-1
    `at::add` launches; here they arrive as separate arguments and are summed by ONE pass of cape_add_n_f32 (k reads, one
    write).  Gradients that autograd reports as None (an unused alias) are skipped."""

    @staticmethod
    def forward(ctx, x, k, slot):
        ctx.k, ctx.slot = k, slot
        ctx.set_materialize_grads(False)
        return tuple(x.view_as(x) for _ in range(k))

    @staticmethod
    def backward(ctx, *grads):
        ctx.slot.buf = None                                  # every consumer has run: a later pass (retain_graph) starts afresh
        gs, seen = [], set()
        for g in grads:                                      # consumers that accumulated into the slot's buffer report it more than once
            if g is not None and (g.data_ptr(), g.numel()) not in seen:
                seen.add((g.data_ptr(), g.numel()))
                gs.append(g)
        if not gs:
            return None, None, None
        if len(gs) > 1 and len(gs) <= 8 and not all(g.is_contiguous() for g in gs) and all(_row_strided(g) for g in gs):
            return ops.add_n_rows(gs), None, None            # a summand is a column block of a wider buffer: summed where it lies
        gs = [_c(g) for g in gs]
        out = gs[0]
        for i in range(0, len(gs) - 1, 7):                  # 8 sources per launch
            out = ops.add_n([out] + gs[1 + i:8 + i]) if len(gs) > 1 else out
        return out, None, None


def _row_strided(g):
    if g.dim() < 2 or g.stride(-1) != 1 or g.shape[-1] % 4 or g.data_ptr() % 16 or g.stride(-2) % 4:
        return False
    st, sh = g.stride(), g.shape
    return all(st[i] == st[i + 1] * sh[i + 1] for i in range(len(sh) - 2))


def fanout(x, k):
    """k aliases of x whose gradients are summed by one HIP launch (no-op outside autograd or for k == 1)."""
    if k == 1 or not (torch.is_grad_enabled() and x.requires_grad):
        return (x,) * k
    slot = _Slot()
    outs = FanOutFn.apply(x, k, slot)
    for o in outs:
        o._cape_slot = slot                                  # consumers find the shared gradient slot on their input (see _Slot)
    return outs


# ------------------------------------------------------------------------------------------------
# pieces of the bidirectional cross-attention blocks (models/bixattn.py): exact GELU, LayerScale residual, attention cores over
# [r | v] projections.  Dropout-free (the reference never trains these blocks; the fixtures are taken with every rate at 0)
# ------------------------------------------------------------------------------------------------
class GeluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _c(x)
        ctx.save_for_backward(x)
        return ops.gelu(x)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return ops.gelu_bwd(x, _c(g))


def gelu(x):
    return GeluFn.apply(x)


class ScaleResidualFn(torch.autograd.Function):
    """out = x + gamma * y (gamma per channel, or None = 1; x None = 0)."""

    @staticmethod
    def forward(ctx, x, y, gamma):
        y = _c(y)
        ctx.has_x = x is not None
        ctx.save_for_backward(y, gamma)
        ctx.gref = gamma
        return ops.scale_residual(_c(x) if x is not None else torch.zeros_like(y), y, gamma)

    @staticmethod
    def backward(ctx, g):
        y, gamma = ctx.saved_tensors
        g = _c(g)
        dx = g if ctx.has_x else None
        if gamma is None:
            return dx, g, None
        pg = _ParamGrads((ctx.gref,))
        dy = ops.scale_residual_bwd(g, y, gamma, pg.bufs[0])
        return (dx, dy) + pg.result()


def scale_residual(x, y, gamma=None):
    return ScaleResidualFn.apply(x, y, gamma)


class BiAttnCoreFn(torch.autograd.Function):
    """Both directions of bixattn.py:52-88 over rv_l = [r_l | v_l] (B, Nl, 2D) and rv_p = [r_p | v_p] (B, Np, 2D):
        lat = softmax_p(scale r_l r_p^T) v_p      pat = softmax_l(scale r_p r_l^T) v_l
    Backward: each direction is one pass of the attention backward kernels writing into column blocks of d_rv_l / d_rv_p; the two
    contributions to d r_l (query of one direction, key of the other) and to d r_p are added in place."""

    @staticmethod
    def forward(ctx, rv_l, rv_p, nheads, scale):
        rv_l, rv_p = _c(rv_l), _c(rv_p)
        B, Nl, D2 = rv_l.shape
        Np, D = rv_p.shape[1], D2 // 2
        ctx.route = "scalar"
        lat, s1 = ops.attn_core_fwd(ctx.route, rv_l[..., :D], rv_p[..., :D], rv_p[..., D:], B, nheads, Nl, Np, scale)
        pat, s2 = ops.attn_core_fwd(ctx.route, rv_p[..., :D], rv_l[..., :D], rv_l[..., D:], B, nheads, Np, Nl, scale)
        ctx.save_for_backward(rv_l, rv_p, lat, pat, *s1, *s2)
        ctx.meta = (nheads, scale)
        return lat, pat

    @staticmethod
    def backward(ctx, d_lat, d_pat):
        rv_l, rv_p, lat, pat, *saved = ctx.saved_tensors
        s1, s2 = saved[:len(saved) // 2], saved[len(saved) // 2:]
        nheads, scale = ctx.meta
        B, Nl, D2 = rv_l.shape
        Np, D = rv_p.shape[1], D2 // 2
        d_l, d_p = torch.empty_like(rv_l), torch.empty_like(rv_p)
        t_l, t_p = torch.empty_like(rv_l), torch.empty_like(rv_p)     # (only the r halves are used: same row stride as the inputs)
        ops.attn_core_bwd(ctx.route, s1, _c(d_lat), rv_l[..., :D], rv_p[..., :D], rv_p[..., D:], lat, d_l[..., :D], d_p[..., :D],
                          d_p[..., D:], B, nheads, Nl, Np, scale)
        ops.attn_core_bwd(ctx.route, s2, _c(d_pat), rv_p[..., :D], rv_l[..., :D], rv_l[..., D:], pat, t_p[..., :D], t_l[..., :D],
                          d_l[..., D:], B, nheads, Np, Nl, scale)
        ops.add_n_rows([d_l[..., :D], t_l[..., :D]], out=d_l[..., :D])
        ops.add_n_rows([d_p[..., :D], t_p[..., :D]], out=d_p[..., :D])
        return d_l, d_p, None, None


def bi_attn_core(rv_l, rv_p, nheads, scale):
    return BiAttnCoreFn.apply(rv_l, rv_p, nheads, float(scale))


class AttnKVFn(torch.autograd.Function):
    """One direction (bixattn.py:90-119): out = softmax(scale r_q r_k^T) v_k with [r_k | v_k] = rv_kv (B, Nk, 2D)."""

    @staticmethod
    def forward(ctx, r_q, rv_kv, nheads, scale):
        r_q, rv_kv = _c(r_q), _c(rv_kv)
        B, Nq, D = r_q.shape
        Nk = rv_kv.shape[1]
        ctx.route = "scalar"
        out, saved = ops.attn_core_fwd(ctx.route, r_q, rv_kv[..., :D], rv_kv[..., D:], B, nheads, Nq, Nk, scale)
        ctx.save_for_backward(r_q, rv_kv, out, *saved)
        ctx.meta = (nheads, scale)
        return out

    @staticmethod
    def backward(ctx, d_out):
        r_q, rv_kv, out, *saved = ctx.saved_tensors
        nheads, scale = ctx.meta
        B, Nq, D = r_q.shape
        Nk = rv_kv.shape[1]
        dq, dkv = torch.empty_like(r_q), torch.empty_like(rv_kv)
        ops.attn_core_bwd(ctx.route, saved, _c(d_out), r_q, rv_kv[..., :D], rv_kv[..., D:], out, dq, dkv[..., :D], dkv[..., D:], B, nheads,
                          Nq, Nk, scale)
        return dq, dkv, None, None


def attn_kv(r_q, rv_kv, nheads, scale):
    return AttnKVFn.apply(r_q, rv_kv, nheads, float(scale))


# ------------------------------------------------------------------------------------------------
# input_proj GroupNorm of all levels, written straight into the flattened token buffer
# ------------------------------------------------------------------------------------------------
class LevelGroupNormFn(torch.autograd.Function):
    """xs: L tensors (N, h_l, w_l, C) NHWC; returns src_flatten (N, S, C)."""

    @staticmethod
    def forward(ctx, geo, *args):
        L = geo.L
        xs, gammas, betas = args[:L], args[L:2 * L], args[2 * L:3 * L]
        N, C = xs[0].shape[0], xs[0].shape[-1]
        out = torch.empty(N, geo.S, C, dtype=torch.float32, device=xs[0].device)
        stats = []
        xs = [_c(x) for x in xs]
        for l, x in enumerate(xs):
            h, w = geo.shapes[l]
            assert x.shape[1] == h and x.shape[2] == w
            stats.append(ops.groupnorm_fwd(x, gammas[l], betas[l], out[:, geo.starts[l]:], geo.S * C, N, h * w, C))
        ctx.geo = geo
        ctx.refs = (tuple(gammas), tuple(betas))
        ctx.save_for_backward(*xs, *gammas, *[s for st in stats for s in st])
        return out

    @staticmethod
    def backward(ctx, d_out):
        geo = ctx.geo
        L = geo.L
        sv = ctx.saved_tensors
        xs, gammas, st = sv[:L], sv[L:2 * L], sv[2 * L:]
        d_out = _c(d_out)
        N, S, C = d_out.shape
        dxs, dgs, dbs = [], [], []
        for l in range(L):
            h, w = geo.shapes[l]
            pg = _ParamGrads((ctx.refs[0][l], ctx.refs[1][l]))
            dx = ops.groupnorm_bwd(d_out[:, geo.starts[l]:], S * C, xs[l], gammas[l], st[2 * l], st[2 * l + 1], *pg.bufs, N,
                                   h * w, C)
            dg, db = pg.result()
            dxs.append(dx); dgs.append(dg); dbs.append(db)
        return (None, *dxs, *dgs, *dbs)


def level_groupnorm(geo, xs, gammas, betas):
    return LevelGroupNormFn.apply(geo, *xs, *gammas, *betas)


_SINE_CACHE = {}


class LevelPosFn(torch.autograd.Function):
    """Image sine position embedding + level_embed, flattened (N, S, C)."""

    @staticmethod
    def forward(ctx, geo, level_embed, *masks_u8):
        N = masks_u8[0].shape[0]
        C = level_embed.shape[1]
        out = torch.empty(N, geo.S, C, dtype=torch.float32, device=level_embed.device)
        # unpadded batches hand in the cached all-False masks (util/misc.cached_zero_mask): the sine part is then a constant of the
        # geometry, kept once (44.5 MB at 32 x 1360 x 256) -- a step only adds the trainable level_embed rows to it
        key = (tuple(m.data_ptr() for m in masks_u8), tuple(geo.shapes), N, C, str(level_embed.device))
        sine = _SINE_CACHE.get(key) if all(getattr(m, "_cape_all_false", False) for m in masks_u8) else None
        if sine is None:
            target = out
            if all(getattr(m, "_cape_all_false", False) for m in masks_u8) and not capturing():
                target = torch.empty_like(out)
            zero_row = torch.zeros(C, dtype=torch.float32, device=level_embed.device) if target is not out else None
            for l, m in enumerate(masks_u8):
                h, w = geo.shapes[l]
                ops.pos_sine_level(_c(m), zero_row if zero_row is not None else level_embed[l], target[:, geo.starts[l]:], geo.S * C, N, h, w, C)
            if target is not out:
                if len(_SINE_CACHE) >= 8:
                    _SINE_CACHE.pop(next(iter(_SINE_CACHE)))
                _SINE_CACHE[key] = sine = target
        if sine is not None:
            ops.level_embed_add(sine, _c(level_embed), geo, out)
        ctx.geo = geo
        ctx.N = N
        ctx.le_ref = level_embed
        return out

    @staticmethod
    def backward(ctx, d_pos):
        geo, N = ctx.geo, ctx.N
        d_pos = _c(d_pos)
        C = d_pos.shape[-1]
        pg = _ParamGrads((ctx.le_ref,))
        for l in range(geo.L):
            h, w = geo.shapes[l]
            ops.colsum(d_pos[0, geo.starts[l]:], h * w, C, pg.bufs[0][l], nbatch=N, batch_stride=geo.S * C)
        return (None,) + pg.result() + (None,) * geo.L


def level_pos(geo, level_embed, masks_u8):
    return LevelPosFn.apply(geo, level_embed, *masks_u8)


# ------------------------------------------------------------------------------------------------
# MSDA core
# ------------------------------------------------------------------------------------------------
class MSDAFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, value, offw, ref, geo, P):
        value, offw, ref = _c(value), _c(offw), _c(ref)
        N, Lq = offw.shape[0], offw.shape[1]
        out = ops.msda_fwd(value, offw, ref, geo, N, Lq, P)
        ctx.save_for_backward(value, offw, ref)
        ctx.meta = (geo, N, Lq, P)
        return out

    @staticmethod
    def backward(ctx, d_out):
        value, offw, ref = ctx.saved_tensors
        geo, N, Lq, P = ctx.meta
        dv, do, dr = ops.msda_bwd(_c(d_out), value, offw, ref, geo, N, Lq, P, need_ref_grad=ctx.needs_input_grad[2])
        return dv, do, dr, None, None


def msda(value, offw, ref, geo, P=4):
    return MSDAFn.apply(value, offw, ref, geo, P)


# ------------------------------------------------------------------------------------------------
# nn.MultiheadAttention (in_proj + core + out_proj) as one node
# ------------------------------------------------------------------------------------------------
def _from_row(t, r):
    return t if (t is None or r == 0) else t[r:]


def _col_blocks(groups, bufs, C):
    """The q, k, v column blocks of the groups' buffers (see MHAFn)."""
    return [buf[..., j * C:(j + 1) * C] for (_, w, *_), buf in zip(groups, bufs) for j in range(w)]


class MHAFn(torch.autograd.Function):
    """The in-projection runs as a list of GROUPS (r, w, dup): w consecutive C-row blocks of in_proj_weight from block r on, applied
    to the r-th input (q_in, k_in, v_in = inputs 0, 1, 2) in ONE product whose result buffer (N, L, wC) holds the w projections
    as column blocks.  A group costs one product forward and two backward (weight and data gradient).  Projections of the same
    input share a group (the support encoder's self-attention, q = k = v: one group, N = 768; cross-attention onto the support
    features, k = v: two groups, N = 256 and 512) unless the attention route is "mm"; the scalar attention kernels take the
    column views (row stride 3C / 2C) as they are.  dup: the input is the tensor that also came in as k."""

    @staticmethod
    def forward(ctx, q_in, k_in, v_in, in_w, in_b, out_w, out_b, nheads, mask_mode, kpm_u8, dropout_p, rng_stream):
        ins = q_in, k_in, v_in = _c(q_in), _c(k_in), _c(v_in)
        N, Lq, C = q_in.shape
        Lk = k_in.shape[1]
        dev = q_in.device
        scale = (C // nheads) ** -0.5
        rng = Runtime.get_rng(dev) if dropout_p > 0 else None
        ctx.route = ops.attn_route(N, nheads, Lq, Lk, flash=False)
        if ctx.route != "mm" and k_in is v_in:
            layout = ((0, 3),) if q_in is k_in else ((0, 1), (1, 2))
        else:
            layout = ((0, 1), (1, 1), (2, 1))
        ctx.groups = tuple((r, w, r != 1 and ins[r] is k_in) for r, w in layout)
        bufs = [torch.empty(N, ins[r].shape[1], w * C, dtype=torch.float32, device=dev) for r, w in layout]
        for (r, w), buf in zip(layout, bufs):
            ops.gemm(ins[r].view(-1, C), _from_row(in_w, r * C), buf, N * ins[r].shape[1], w * C, C, bias=_from_row(in_b, r * C))
        q, k, v = _col_blocks(layout, bufs, C)
        O, saved = ops.attn_core_fwd(ctx.route, q, k, v, N, nheads, Lq, Lk, scale, mask_mode=mask_mode, kpm=kpm_u8, dropout_p=dropout_p,
                                     rng=rng, rng_stream=rng_stream)
        out = torch.empty(N, Lq, C, dtype=torch.float32, device=dev)
        ops.gemm(O.view(-1, C), out_w, out, N * Lq, C, C, bias=out_b)
        ctx.save_for_backward(q_in, k_in, v_in, in_w, out_w, q, k, v, O, kpm_u8, *saved)
        ctx.refs = (in_w, in_b, out_w, out_b)
        ctx.slot_q = _slot_of(q_in)
        ctx.meta = (nheads, mask_mode, dropout_p, rng_stream, scale)
        return out

    @staticmethod
    def backward(ctx, d_out):
        q_in, k_in, v_in, in_w, out_w, q, k, v, O, kpm, *saved = ctx.saved_tensors
        nheads, mask_mode, p, stream, scale = ctx.meta
        ins = q_in, k_in, v_in
        N, Lq, C = q_in.shape
        Lk = k_in.shape[1]
        dev = d_out.device
        d_out2 = _c(d_out).view(-1, C)
        Mq = N * Lq
        dO = torch.empty(Mq, C, dtype=torch.float32, device=dev)
        ops.gemm(d_out2, out_w, dO, Mq, C, C, a_mode=0, b_mode=1)
        pg = _ParamGrads(ctx.refs)
        d_in_w, d_in_b, d_out_w, d_out_b = pg.bufs
        with pg.side(d_out2, O):
            pg.gemm(d_out2, O.view(-1, C), d_out_w, C, C, Mq, a_mode=1, b_mode=1, accumulate=True,
                    split_k=ops.pick_split_k(C, C, Mq), colsum_out=d_out_b)
        # gradients in the layout of the projection results: one buffer per group, dq / dk / dv its column blocks
        dbufs = [torch.empty(N, ins[r].shape[1], w * C, dtype=torch.float32, device=dev) for r, w, _ in ctx.groups]
        dq, dk, dv = _col_blocks(ctx.groups, dbufs, C)
        rng = Runtime.get_rng(dev) if p > 0 else None
        ops.attn_core_bwd(ctx.route, saved, dO.view(N, Lq, C), q, k, v, O, dq, dk, dv, N, nheads, Lq, Lk, scale, mask_mode=mask_mode,
                          kpm=kpm, dropout_p=p, rng=rng, rng_stream=stream)
        pairs = list(zip(ctx.groups, dbufs))
        with pg.side(*dbufs, q_in, k_in, v_in):
            for (r, w, _), g in pairs:                       # [d heads of the group]^T x: one product for its stacked in_proj rows
                M = N * ins[r].shape[1]
                pg.gemm(g.view(-1, w * C), ins[r].view(-1, C), _from_row(d_in_w, r * C), w * C, C, M, a_mode=1, b_mode=1, lda=w * C,
                        accumulate=True, split_k=ops.pick_split_k(w * C, C, M), colsum_out=_from_row(d_in_b, r * C))
        d_in_w, d_in_b, d_out_w, d_out_b = pg.result()
        # input gradients, d x = [d heads of the group] . its in_proj rows (K = wC), the key side first: the product of a tensor
        # that also came in as k adds into d k_in (GEMM epilogue C += ...) and reports None; any other gradient reports through
        # the first slot of its group that needs one
        d_ins, dk_in = [None, None, None], None
        for (r, w, dup), g in pairs[1:] + pairs[:1]:
            live = [j for j in range(r, r + w) if ctx.needs_input_grad[j]]
            if not live:
                continue
            if dup and dk_in is not None:
                dst, acc = dk_in, True
            else:
                if r == 0 and len(pairs) == 2:               # (the query of cross-attention onto k = v: a fan-out consumer)
                    dst, acc = _grad_target(ctx.slot_q, ins[r].shape, dev)
                else:
                    dst, acc = torch.empty(ins[r].shape, dtype=torch.float32, device=dev), False
                d_ins[live[0]] = dst
            ops.gemm(g.view(-1, w * C), _from_row(in_w, r * C), dst, N * ins[r].shape[1], C, w * C, a_mode=0, b_mode=1, accumulate=acc)
            if live[0] == 1:
                dk_in = dst
        return (*d_ins, d_in_w, d_in_b, d_out_w, d_out_b, None, None, None, None, None)


class DecSelfAttnFn(torch.autograd.Function):
    """The decoder layer's causal self-attention block (deformable_transformer_v2.py:323-341) as ONE node:
        q = attn_q(tgt) + query_pos ; k = attn_k(tgt) ; v = attn_v(tgt) ; nn.MultiheadAttention(q, k, v, causal mask)
    Round 2 ran it as 3 + 3 projection launches around the attention core (and 3 + 3 data-gradient launches, 7 weight-gradient
    launches and a 4-way gradient sum in the backward).  Here: the three bias-free projections are one product over the stacked
    (3C, C) weight rows with the `+ query_pos` epilogue on the q columns (attn_q / attn_k / attn_v sit back to back in the flat
    arena); the three in_proj blocks are one batch-3 launch (block i multiplies columns [iC, (i+1)C) of the first product);
    the backward mirrors it (one batch-3 data gradient, ONE K = 3C product for d tgt -- the gradient sum over the three
    consumers of `tgt` happens inside the contraction), and the seven weight gradients join the deferred groups."""

    @staticmethod
    def forward(ctx, tgt, pos, wq, wk, wv, in_w, in_b, out_w, out_b, nheads, dropout_p, rng_stream):
        N, L, C = tgt.shape
        M = N * L
        dev = tgt.device
        x, pos2 = _c(tgt).view(M, C), _c(pos).view(M, C)
        stacked = _adjacent(wq, wk) and _adjacent(wk, wv)
        qkv1 = torch.empty(M, 3 * C, dtype=torch.float32, device=dev)
        if stacked:
            ops.gemm(x, torch.as_strided(wq, (3 * C, C), (C, 1)), qkv1, M, 3 * C, C, residual=pos2, ldr=C, res_cols=C)
        else:
            ops.gemm(x, wq, qkv1, M, C, C, ldc=3 * C, residual=pos2, ldr=C)
            ops.gemm(x, wk, qkv1[:, C:], M, C, C, ldc=3 * C)
            ops.gemm(x, wv, qkv1[:, 2 * C:], M, C, C, ldc=3 * C)
        qkv2 = torch.empty(N, L, 3 * C, dtype=torch.float32, device=dev)
        ops.gemm(qkv1, in_w, qkv2, M, C, C, lda=3 * C, ldb=C, ldc=3 * C, bias=in_b,
                 batch=(3, 3, 0, C, 0, C * C, 0, C), bias_strides=(0, C))
        q, k, v = qkv2[..., :C], qkv2[..., C:2 * C], qkv2[..., 2 * C:]
        scale = (C // nheads) ** -0.5
        rng = Runtime.get_rng(dev) if dropout_p > 0 else None
        ctx.route = ops.attn_route(N, nheads, L, L, flash=True)
        O, saved = ops.attn_core_fwd(ctx.route, q, k, v, N, nheads, L, L, scale, mask_mode=1, dropout_p=dropout_p, rng=rng,
                                     rng_stream=rng_stream)
        out = torch.empty(N, L, C, dtype=torch.float32, device=dev)
        ops.gemm(O.view(M, C), out_w, out, M, C, C, bias=out_b)
        ctx.save_for_backward(x, wq, wk, wv, in_w, out_w, qkv1, qkv2, O, *saved)
        ctx.refs = (wq, wk, wv, in_w, in_b, out_w, out_b)
        ctx.meta = (nheads, dropout_p, rng_stream, scale, stacked, N, L, C)
        ctx.slot = _slot_of(tgt)
        return out

    @staticmethod
    def backward(ctx, d_out):
        x, wq, wk, wv, in_w, out_w, qkv1, qkv2, O, *saved = ctx.saved_tensors
        nheads, p, stream, scale, stacked, N, L, C = ctx.meta
        M = N * L
        dev = d_out.device
        d_out2 = _c(d_out).view(M, C)
        dO = torch.empty(M, C, dtype=torch.float32, device=dev)
        ops.gemm(d_out2, out_w, dO, M, C, C, a_mode=0, b_mode=1)
        dqkv2 = torch.empty(N, L, 3 * C, dtype=torch.float32, device=dev)
        dq, dk, dv = dqkv2[..., :C], dqkv2[..., C:2 * C], dqkv2[..., 2 * C:]
        q, k, v = qkv2[..., :C], qkv2[..., C:2 * C], qkv2[..., 2 * C:]
        rng = Runtime.get_rng(dev) if p > 0 else None
        ops.attn_core_bwd(ctx.route, saved, dO.view(N, L, C), q, k, v, O, dq, dk, dv, N, nheads, L, L, scale, mask_mode=1, dropout_p=p,
                          rng=rng, rng_stream=stream)
        dqkv1 = torch.empty(M, 3 * C, dtype=torch.float32, device=dev)
        ops.gemm(dqkv2.view(M, 3 * C), in_w, dqkv1, M, C, C, a_mode=0, b_mode=1, lda=3 * C, ldb=C, ldc=3 * C,
                 batch=(3, 3, 0, C, 0, C * C, 0, C))
        need_x, need_pos = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dx = None
        if need_x:
            dx, acc = _grad_target(ctx.slot, (N, L, C), dev)
            if stacked:
                ops.gemm(dqkv1, torch.as_strided(wq, (3 * C, C), (C, 1)), dx, M, C, 3 * C, a_mode=0, b_mode=1, accumulate=acc)
            else:
                for i, w in enumerate((wq, wk, wv)):
                    ops.gemm(dqkv1[:, i * C:], w, dx, M, C, C, a_mode=0, b_mode=1, lda=3 * C, accumulate=acc or i > 0)

        pg = _ParamGrads(ctx.refs)
        d_wq, d_wk, d_wv, d_in_w, d_in_b, d_out_w, d_out_b = pg.bufs
        with pg.side(d_out2, O, dqkv2, qkv1, dqkv1, x):
            Mv = dqkv2.view(M, 3 * C)
            pg.gemm(d_out2, O.view(M, C), d_out_w, C, C, M, a_mode=1, b_mode=1, accumulate=True, split_k=ops.pick_split_k(C, C, M),
                    colsum_out=d_out_b)
            for i, dw in enumerate((d_wq, d_wk, d_wv)):
                pg.gemm(Mv[:, i * C:], qkv1[:, i * C:], d_in_w[i * C:], C, C, M, a_mode=1, b_mode=1, lda=3 * C, ldb=3 * C, accumulate=True,
                        split_k=ops.pick_split_k(C, C, M), colsum_out=d_in_b[i * C:])
                pg.gemm(dqkv1[:, i * C:], x, dw, C, C, M, a_mode=1, b_mode=1, lda=3 * C, ldb=C, accumulate=True,
                        split_k=ops.pick_split_k(C, C, M))
        dpos = dqkv1[:, :C].view(N, L, C) if need_pos else None      # (a row-strided view of the wide gradient)
        return (dx, dpos) + pg.result() + (None, None, None)


def dec_self_attn(tgt, pos, wq, wk, wv, in_w, in_b, out_w, out_b, nheads=8, dropout_p=0.0, rng_stream=0):
    return DecSelfAttnFn.apply(tgt, pos, wq, wk, wv, in_w, in_b, out_w, out_b, nheads, float(dropout_p), int(rng_stream))


def mha(q_in, k_in, v_in, in_w, in_b, out_w, out_b, nheads=8, mask_mode=0, kpm_u8=None, dropout_p=0.0, rng_stream=0):
    return MHAFn.apply(q_in, k_in, v_in, in_w, in_b, out_w, out_b, nheads, mask_mode, kpm_u8, float(dropout_p), int(rng_stream))


# ------------------------------------------------------------------------------------------------
# decoder embedding / reference-point ops
# ------------------------------------------------------------------------------------------------
class TokenEmbedFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table, pad_idx, s11, s21, s12, s22, dx1, dx2, dy1, dy2):
        shape = s11.shape
        seqs = [_c(s).view(-1) for s in (s11, s21, s12, s22)]
        deltas = [_c(d).view(-1) for d in (dx1, dx2, dy1, dy2)]
        out = ops.token_embed_fwd(table, seqs, deltas)
        ctx.save_for_backward(*seqs, *deltas)
        ctx.t_ref = table
        ctx.meta = (table.shape, pad_idx)
        return out.view(*shape, table.shape[1])

    @staticmethod
    def backward(ctx, d_out):
        sv = ctx.saved_tensors
        tshape, pad_idx = ctx.meta
        pg = _ParamGrads((ctx.t_ref,))
        ops.token_embed_bwd(_c(d_out).view(-1, tshape[1]), sv[:4], sv[4:], pg.bufs[0], pad_idx if pad_idx is not None else -1)
        return pg.result() + (None,) * 9


def token_embed(table, pad_idx, s11, s21, s12, s22, dx1, dx2, dy1, dy2):
    return TokenEmbedFn.apply(table, pad_idx, s11, s21, s12, s22, dx1, dx2, dy1, dy2)


class QuerySineFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ref):
        ref = _c(ref)
        ctx.save_for_backward(ref)
        return ops.query_sine_fwd(ref).view(*ref.shape[:-1], 256)

    @staticmethod
    def backward(ctx, d_out):
        (ref,) = ctx.saved_tensors
        return ops.query_sine_bwd(_c(d_out).view(-1, 256), ref).view_as(ref)


def query_sine(ref):
    return QuerySineFn.apply(ref)


class RefineFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, delta, ref):
        delta, ref = _c(delta), _c(ref)
        out = ops.refine_fwd(delta, ref)
        ctx.save_for_backward(out, ref)
        return out

    @staticmethod
    def backward(ctx, d_new):
        out, ref = ctx.saved_tensors
        d_delta, d_ref = ops.refine_bwd(_c(d_new), out, ref)
        return d_delta, d_ref


def refine(delta, ref):
    return RefineFn.apply(delta, ref)


class SigmoidFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        y = ops.sigmoid_fwd(_c(x))
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        return ops.sigmoid_bwd(_c(dy), y)


def sigmoid(x):
    return SigmoidFn.apply(x)


class RefScaleFn(torch.autograd.Function):
    """ref (N, Lq, 2) * valid_ratios (N, L, 2) -> (N, Lq, L, 2)"""

    @staticmethod
    def forward(ctx, ref, valid_ratios):
        ref, vr = _c(ref), _c(valid_ratios)
        N, Lq, _ = ref.shape
        L = vr.shape[1]
        ctx.save_for_backward(vr)
        ctx.meta = (N, Lq, L)
        return ops.ref_scale_fwd(ref, vr, Lq, L).view(N, Lq, L, 2)

    @staticmethod
    def backward(ctx, d):
        (vr,) = ctx.saved_tensors
        N, Lq, L = ctx.meta
        return ops.ref_scale_bwd(_c(d), vr, Lq, L).view(N, Lq, 2), None


def ref_scale(ref, valid_ratios):
    return RefScaleFn.apply(ref, valid_ratios)


# ------------------------------------------------------------------------------------------------
# support encoder pieces
# ------------------------------------------------------------------------------------------------
class SupportEmbedFn(torch.autograd.Function):
    """coords (N,P,2) -> h = relu(Linear_2->C(coords)) (N,P,C), pe = sine2d + pe1d (N,P,C; no gradient)."""

    @staticmethod
    def forward(ctx, coords, W0, b0, pe1d):
        coords = _c(coords)
        N, P, _ = coords.shape
        C = W0.shape[0]
        h, pe = ops.support_embed_fwd(coords, W0, b0, pe1d, N, P, C)
        ctx.save_for_backward(h, coords)
        ctx.refs = (W0, b0)
        ctx.meta = (N, P, C)
        ctx.mark_non_differentiable(pe)
        ctx.set_materialize_grads(False)
        return h.view(N, P, C), pe.view(N, P, C)

    @staticmethod
    def backward(ctx, d_h, _d_pe):
        if d_h is None:
            return None, None, None, None
        h, coords = ctx.saved_tensors
        N, P, C = ctx.meta
        pg = _ParamGrads(ctx.refs)
        ops.support_embed_bwd(_c(d_h).view(-1, C), h, coords, *pg.bufs, N, P, C)
        return (None,) + pg.result() + (None,)


def support_embed(coords, W0, b0, pe1d):
    return SupportEmbedFn.apply(coords, W0, b0, pe1d)


class GCNAggFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, adj):
        y = _c(y)
        N, P, C2 = y.shape
        out = ops.gcn_aggregate_fwd(y, adj, N, P, C2 // 2)
        ctx.save_for_backward(out, adj)
        return out

    @staticmethod
    def backward(ctx, d_out):
        out, adj = ctx.saved_tensors
        N, P, C = out.shape
        return ops.gcn_aggregate_bwd(_c(d_out), out, adj, N, P, C), None


def gcn_aggregate(y, adj):
    return GCNAggFn.apply(y, adj)


class ZeroRowsFn(torch.autograd.Function):
    """x[rowmask] = 0 (the all-masked guard of the support encoder); gradient is masked the same way."""

    @staticmethod
    def forward(ctx, x, rowmask_u8):
        x = _c(x).clone()
        ops.zero_rows(x, rowmask_u8)
        ctx.save_for_backward(rowmask_u8)
        return x

    @staticmethod
    def backward(ctx, g):
        (rm,) = ctx.saved_tensors
        g = _c(g).clone()
        ops.zero_rows(g, rm)
        return g, None


def zero_rows(x, rowmask_u8):
    return ZeroRowsFn.apply(x, rowmask_u8)


# ------------------------------------------------------------------------------------------------
# default (non-geometric) support encoder pieces (models/support_encoder.py)
# ------------------------------------------------------------------------------------------------
class LegacyCoordEmbedFn(torch.autograd.Function):
    """coords (N,P,2) -> relu(Linear_2->C(coords)) (N,P,C); the coordinate gradient is produced when asked for."""

    @staticmethod
    def forward(ctx, coords, W0, b0):
        coords = _c(coords)
        N, P, _ = coords.shape
        h = ops.legacy_coord_embed_fwd(coords, W0, b0)
        ctx.save_for_backward(h, coords, W0)
        ctx.refs = (W0, b0)
        return h.view(N, P, -1)

    @staticmethod
    def backward(ctx, d_h):
        h, coords, W0 = ctx.saved_tensors
        pg = _ParamGrads(ctx.refs, ctx.needs_input_grad[1:3])
        dW0, db0 = pg.bufs
        if dW0 is None or db0 is None:                  # (the kernel takes both or neither)
            dW0 = dW0 if dW0 is not None else torch.zeros_like(W0)
            db0 = db0 if db0 is not None else torch.zeros(W0.shape[0], dtype=torch.float32, device=W0.device)
        dc = ops.legacy_coord_embed_bwd(_c(d_h), h, coords, W0, dW0, db0, want_dcoords=ctx.needs_input_grad[0])
        return (dc.view_as(coords) if dc is not None else None,) + pg.result()


def legacy_coord_embed(coords, W0, b0):
    return LegacyCoordEmbedFn.apply(coords, W0, b0)


class EdgeCatFn(torch.autograd.Function):
    """[h W2^T + b2 | edge_info] (N, P, 2C): the second coord_embedding linear writes the left half (GEMM with row stride 2C),
    cape_support_edge_info_fwd the right half -- `torch.cat([coord_emb, edge_info])` of support_encoder.py:79 without a copy."""

    @staticmethod
    def forward(ctx, h, W2, b2, E, edges, start):
        h = _c(h)
        N, P, K = h.shape
        C = W2.shape[0]
        M = N * P
        h2 = h.view(M, K)
        cat = torch.empty(N, P, 2 * C, dtype=torch.float32, device=h.device)
        cat2 = cat.view(M, 2 * C)
        ops.gemm(h2, W2, cat2, M, C, K, ldb=W2.stride(0), bias=b2, ldc=2 * C)
        scale, has, _ = ops.support_edge_info_fwd(edges, start, E, cat2[:, C:], N, P)
        ctx.save_for_backward(h2, W2, scale, has)
        ctx.refs = (W2, b2, E)
        ctx.meta = (N, P, K, C)
        return cat

    @staticmethod
    def backward(ctx, d_cat):
        h2, W2, scale, has = ctx.saved_tensors
        N, P, K, C = ctx.meta
        M = N * P
        g = _c(d_cat).view(M, 2 * C)
        dh = None
        if ctx.needs_input_grad[0]:
            dh = torch.empty(M, K, dtype=torch.float32, device=g.device)
            ops.gemm(g, W2, dh, M, K, C, a_mode=0, b_mode=1, lda=2 * C, ldb=W2.stride(0))
            dh = dh.view(N, P, K)
        pg = _ParamGrads(ctx.refs, ctx.needs_input_grad[1:4])
        dW2, db2, dE = pg.bufs
        if dE is not None:
            ops.support_edge_info_bwd(g[:, C:], scale, has, dE)
        with pg.side(g, h2):
            if dW2 is not None:
                pg.gemm(g, h2, dW2, C, K, M, a_mode=1, b_mode=1, lda=2 * C, ldb=K, ldc=dW2.stride(0), accumulate=True,
                        split_k=ops.pick_split_k(C, K, M), colsum_out=db2)
            elif db2 is not None:
                ops.colsum(g, M, C, db2, ldx=2 * C)
        return (dh,) + pg.result() + (None, None)


def edge_cat(h, W2, b2, E, edges, start):
    return EdgeCatFn.apply(h, W2, b2, E, edges, start)


class PEDropoutFn(torch.autograd.Function):
    """dropout(x + pe[:P]) -- PositionalEncoding1D.forward of support_encoder.py:151-159, in that order."""

    @staticmethod
    def forward(ctx, x, pe, dropout_p, rng_stream):
        x = _c(x)
        rng = Runtime.get_rng(x.device) if dropout_p > 0 else None
        out = ops.pe_dropout_fwd(x, pe, x.shape[-2], dropout_p, rng, rng_stream)
        ctx.meta = (dropout_p, rng_stream)
        return out

    @staticmethod
    def backward(ctx, g):
        p, stream = ctx.meta
        if p == 0:
            return g, None, None, None
        return ops.pe_dropout_bwd(_c(g), p, Runtime.get_rng(g.device), stream), None, None, None


def pe_dropout(x, pe, dropout_p=0.0, rng_stream=0):
    return PEDropoutFn.apply(x, pe, float(dropout_p), int(rng_stream))


# ------------------------------------------------------------------------------------------------
# criterion
# ------------------------------------------------------------------------------------------------
class LossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, coords, labels, vis_u8, target, class_w, w_ce, w_l1):
        losses, total, dl, dc = ops.loss_fwd_bwd(_c(logits), _c(coords), _c(labels).view(-1), _c(vis_u8).view(-1),
                                                 _c(target).view(-1, 2), class_w, w_ce, w_l1, 1.0)
        ctx.save_for_backward(dl, dc)
        ctx.mark_non_differentiable(losses)
        ctx.set_materialize_grads(False)
        return total.view(()), losses

    @staticmethod
    def backward(ctx, g_total, _g_losses):
        if g_total is None:
            return (None,) * 8
        dl, dc = ctx.saved_tensors
        # scaling by the incoming scalar gradient is glue (1/accumulation_steps)
        return dl * g_total, dc * g_total, None, None, None, None, None, None


def cape_loss(logits, coords, labels, vis_u8, target, class_w, w_ce, w_l1):
    return LossFn.apply(logits, coords, labels, vis_u8, target, class_w, float(w_ce), float(w_l1))
