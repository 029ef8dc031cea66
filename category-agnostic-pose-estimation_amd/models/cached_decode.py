"""KV-cached autoregressive decode behind `RoomFormerV2.forward_inference`: step tiers, per-geometry state, one loop.

A decode step exists in three tiers; `decode_tier` picks one per call and the other two stay as its cross-checks:
  * "per_op": one launch per operation, `TransformerDecoder.decode_step` (the GEMM / attention / MSDA / LayerNorm kernels of
    the teacher-forced pass) + `decode_next_tokens`.  CAPE_DECODE_FUSED=0, or > 64 images where "whole" does not apply;
  * "stage": one launch per stage of a layer (csrc/decode_step.hip: `decode_linear` with the LayerNorms applied on load,
    `decode_tail`) over folded weights (`DecodeWeights`) + `decode_advance`.  <= 64 images where "whole" does not apply;
  * "whole": the step as ONE launch, one block per image (csrc/decode_fused.hip through `ops.DecodeStepPlan`) +
    `decode_advance`.  The default; needs the CAPE layer shape (support attention, 1, 3 or 4 levels x 4 points, dim_feedforward 1024).

A step works on a few rows, i.e. is host-bound, so the steps are captured as hipGraphs -- one per step index, because the
cache row written, the attention length and the output slot are baked into the launch arguments -- over the static buffers
of a `DecodeState`.  Call 1 of a geometry runs eagerly (the warm-up a capture needs), call 2 captures while it decodes, later
calls replay.  Every buffer a captured step points into keeps its storage for the life of the state."""
import os

import torch

from ..hip import ops
from .kv_cache import KVCache, VCache

MIN_LEN = 6            # <eos> is accepted from this step on
WHOLE_STEP_SAMPLES = (4, 12, 16)      # levels x points per head the whole-step kernel is instantiated for (1, 3, 4 levels x 4 points)


def _fold(w_in, w_a):
    """(w_in @ w_a) on the device in exact fp32: the two chained projections of the decoder's self-attention
    (attn_x then MultiheadAttention.in_proj, deformable_transformer_v2.py:323-331) as one weight for inference."""
    out = torch.empty(w_in.shape[0], w_a.shape[1], dtype=torch.float32, device=w_in.device)
    old = ops.get_gemm_precision()
    ops.set_gemm_precision("f32")
    try:
        ops.gemm(w_in, w_a, out, w_in.shape[0], w_a.shape[1], w_in.shape[1], a_mode=0, b_mode=1, ldb=w_a.stride(0))
    finally:
        ops.set_gemm_precision(old)
    return out


class DecodeWeights:
    """Inference-time weights of the fused decode step, rebuilt when any source parameter changed
    (version counter or storage): per layer the folded q|k|v projection (768 x 256) and the concatenated
    sampling_offsets|attention_weights projection (8 * levels * points * 3 rows x 256: 96 / 288 / 384 at 1 / 3 / 4 levels)."""

    def __init__(self, decoder):
        self.decoder, self.key, self.layers = decoder, None, None

    def _sources(self):
        out = []
        for l in self.decoder.layers:
            m = l.cross_attn
            out += [l.attn_q.weight, l.attn_k.weight, l.attn_v.weight, l.self_attn.in_proj_weight, m.sampling_offsets.weight,
                    m.sampling_offsets.bias, m.attention_weights.weight, m.attention_weights.bias]
        return out

    def get(self):
        # (the optimizer kernel updates the flat arenas behind autograd's back -- no `_version` bump: its epoch counter, the one
        # the packed GEMM weights follow, is part of the key)
        key = (ops.PackedWeights.epoch,) + tuple((t.data_ptr(), t._version) for t in self._sources())
        if key != self.key:
            C = self.decoder.layers[0].d_model
            layers = []
            with torch.no_grad():
                for l in self.decoder.layers:
                    W = l.self_attn.in_proj_weight
                    m = l.cross_attn
                    layers.append({
                        "w_qkv": torch.cat([_fold(W[:C], l.attn_q.weight), _fold(W[C:2 * C], l.attn_k.weight),
                                            _fold(W[2 * C:], l.attn_v.weight)], 0).contiguous(),
                        "w_off": torch.cat([m.sampling_offsets.weight, m.attention_weights.weight], 0).contiguous(),
                        "b_off": torch.cat([m.sampling_offsets.bias, m.attention_weights.bias], 0).contiguous()})
            self.layers, self.key = layers, key
        return self.layers


def alloc_decode_workspace(N, n_layers, L, dev, samples_per_head=16):
    """Static per-geometry buffers of the fused step (pre-norm sums p1..p4, projections, per-layer query positions);
    `offw` is a row of the offsets|weights projection: 8 heads x samples_per_head (levels x points) x 3."""
    f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    return {"emb": f(N, 256), "q": f(N, 256), "qs": f(N, 256), "p1": f(N, 256), "p2": f(N, 256), "p3": f(N, 256),
            "p4": [f(N, 256) for _ in range(n_layers)], "offw": f(N, 8 * samples_per_head * 3), "h": f(N, 1024),
            "qpos": [None] + [f(N, 256) for _ in range(n_layers - 1)], "refin": [None] + [f(N, L, 2) for _ in range(n_layers - 1)],
            "ref": [None] + [f(N, 2) for _ in range(n_layers)]}


@torch.no_grad()
def decode_step_fused(decoder, dw, ws, caches, geo, vr, step, qpos0, refin0, ref0, out_logits, out_coords, out_hs):
    """One cached AR step for N images.  ws["emb"] holds the embedding of the step's input tokens; layer 0's query
    position embedding / level-scaled points / reference come from per-call tables (qpos0 (256,) broadcast over rows,
    refin0 (N, L, 2), ref0 (N, 2)), the later layers' from the previous layer's tail kernel.  Writes the step's class
    logits, refined coordinates and last hidden state into slot `step` of the output buffers."""
    layers = decoder.layers
    nl = len(layers)
    N = ws["emb"].shape[0]
    C, H = 256, layers[0].n_heads
    scale = (C // H) ** -0.5
    dim_t = ops.dim_t(ws["emb"].device)
    x_prev, ln_prev = ws["emb"], None                       # input of the layer as (pre-norm rows, LayerNorm to apply on load)
    for l, (layer, w, c) in enumerate(zip(layers, dw, caches)):
        qpos = qpos0.view(1, C).expand(N, C) if l == 0 else ws["qpos"][l]
        refin = refin0 if l == 0 else ws["refin"][l]
        ref = ref0 if l == 0 else ws["ref"][l]
        sa = layer.self_attn
        # q | k | v in one launch (folded projections; `+ query_pos` through in_proj_q), k / v straight into the cache row
        ops.decode_linear(x_prev, w["w_qkv"], [ws["q"], c["k"][:, step], c["v"][:, step]], bias=sa.in_proj_bias, in_ln=ln_prev,
                          X2=qpos, W2=sa.in_proj_weight[:C])
        a, _ = ops.attn_fwd(ws["q"].view(N, 1, C), c["k"], c["v"], N, H, 1, step + 1, scale, mask_mode=0)
        ops.decode_linear(a.view(N, C), sa.out_proj.weight, [ws["p1"]], bias=sa.out_proj.bias, res=x_prev, res_ln=ln_prev)
        ln2 = (layer.norm2.weight, layer.norm2.bias)
        if c.get("sup_k") is not None:
            ca = layer.support_attn
            ops.decode_linear(ws["p1"], ca.in_proj_weight[:C], [ws["qs"]], bias=ca.in_proj_bias[:C], in_ln=ln2)
            P = c["sup_k"].shape[1]
            a2, _ = ops.attn_fwd(ws["qs"].view(N, 1, C), c["sup_k"], c["sup_v"], N, H, 1, P, scale,
                                 mask_mode=2 if c["sup_kpm"] is not None else 0, kpm=c["sup_kpm"])
            ops.decode_linear(a2.view(N, C), ca.out_proj.weight, [ws["p2"]], bias=ca.out_proj.bias, res=ws["p1"], res_ln=ln2)
            t_pre, t_ln = ws["p2"], (layer.norm_support.weight, layer.norm_support.bias)
        else:
            t_pre, t_ln = ws["p1"], ln2
        m = layer.cross_attn
        ops.decode_linear(t_pre, w["w_off"], [ws["offw"]], bias=w["b_off"], in_ln=t_ln, in_add=qpos)
        g = ops.msda_fwd(c["value"], ws["offw"].view(N, 1, -1), refin.view(N, 1, geo.L, 2), geo, N, 1, m.n_points)
        ops.decode_linear(g.view(N, C), m.output_proj.weight, [ws["p3"]], bias=m.output_proj.bias, res=t_pre, res_ln=t_ln)
        ln1 = (layer.norm1.weight, layer.norm1.bias)
        ops.decode_linear(ws["p3"], layer.linear1.weight, [ws["h"]], bias=layer.linear1.bias, in_ln=ln1, relu=True)
        ops.decode_linear(ws["h"], layer.linear2.weight, [ws["p4"][l]], bias=layer.linear2.bias, res=ws["p3"], res_ln=ln1)
        ln3 = (layer.norm3.weight, layer.norm3.bias)
        mlp = tuple((q.weight, q.bias) for q in decoder.coords_embed[l].layers)
        last = l == nl - 1
        ops.decode_tail(ws["p4"][l], ln3, mlp, ref, out_coords[:, step] if last else ws["ref"][l + 1], dim_t, vr=vr,
                        cls_head=(decoder.class_embed[l].weight, decoder.class_embed[l].bias) if last else None,
                        cls_out=out_logits[:, step] if last else None,
                        pos_trans=None if last else (decoder.pos_trans.weight, decoder.pos_trans.bias, decoder.pos_trans_norm.weight,
                                                     decoder.pos_trans_norm.bias),
                        qpos_out=None if last else ws["qpos"][l + 1], refin_out=None if last else ws["refin"][l + 1],
                        hs_out=out_hs[:, step] if last else None)
        x_prev, ln_prev = ws["p4"][l], ln3


def decode_plan(dec, dw, caches, emb, vr, geo, N, seq_len):
    """Descriptor of the whole-step decode kernel: the pointers of every decoder weight, cache and table (ops.DecodeStepPlan)."""
    layers = []
    for l, (layer, w, c) in enumerate(zip(dec.layers, dw, caches)):
        sa, ca, m = layer.self_attn, layer.support_attn, layer.cross_attn
        mlp = dec.coords_embed[l].layers
        layers.append({
            "w_qkv": w["w_qkv"], "b_qkv": sa.in_proj_bias, "w_qin": sa.in_proj_weight[:256], "k_cache": c["k"], "v_cache": c["v"],
            "w_o": sa.out_proj.weight, "b_o": sa.out_proj.bias, "ln2_g": layer.norm2.weight, "ln2_b": layer.norm2.bias,
            "w_sq": ca.in_proj_weight[:256], "b_sq": ca.in_proj_bias[:256], "sup_k": c["sup_k"], "sup_v": c["sup_v"],
            "sup_mask": c["sup_kpm"], "w_so": ca.out_proj.weight, "b_so": ca.out_proj.bias,
            "lns_g": layer.norm_support.weight, "lns_b": layer.norm_support.bias,
            "w_off": w["w_off"], "b_off": w["b_off"], "value": c["value"], "w_mo": m.output_proj.weight, "b_mo": m.output_proj.bias,
            "ln1_g": layer.norm1.weight, "ln1_b": layer.norm1.bias, "w1": layer.linear1.weight, "b1": layer.linear1.bias,
            "w2": layer.linear2.weight, "b2": layer.linear2.bias, "ln3_g": layer.norm3.weight, "ln3_b": layer.norm3.bias,
            "m1w": mlp[0].weight, "m1b": mlp[0].bias, "m2w": mlp[1].weight, "m2b": mlp[1].bias, "m3w": mlp[2].weight, "m3b": mlp[2].bias})
    ce = dec.class_embed[len(dec.layers) - 1]
    return ops.DecodeStepPlan(N, seq_len, geo, dec.layers[0].cross_attn.n_points, dec.layers[0].linear1.weight.shape[0], emb, vr,
                              ops.dim_t(emb.device), (ce.weight, ce.bias),
                              (dec.pos_trans.weight, dec.pos_trans.bias, dec.pos_trans_norm.weight, dec.pos_trans_norm.bias), layers)


def decode_tier(N, P, samples_per_head, ffn_dim, seq_len, S, n_layers, num_classes):
    """"per_op" | "stage" | "whole" (module docstring) for N images with P support keypoints; samples_per_head = levels x
    points of the decoder's MSDA, S = image tokens.  CAPE_DECODE_FUSED=0 / CAPE_DECODE_MEGA=0 step down a tier for A/B."""
    fused = os.environ.get("CAPE_DECODE_FUSED", "1") == "1"
    whole = (fused and os.environ.get("CAPE_DECODE_MEGA", "1") == "1" and P > 0 and samples_per_head in WHOLE_STEP_SAMPLES and ffn_dim == 1024 and
             seq_len <= 1024 and P <= 1024 and S < 65535 and n_layers <= 8 and num_classes <= 8)
    return "whole" if whole else "stage" if fused and N <= 64 else "per_op"      # the launch-per-stage kernels take <= 64 rows


class DecodeState:
    """Static buffers of one batch geometry, the step graphs captured over them and the whole-step descriptor."""

    def __init__(self, model, N, geo, P, has_mask, max_len, dev, tier):
        dec, T0 = model.transformer.decoder, model.query_embed.weight.shape[0]
        self.N, self.geo, self.P, self.max_len, self.tier = N, geo, P, max_len, tier
        self.calls, self.graphs, self.pool, self.plan, self.weights_at = 0, {}, None, None, None
        self.vr = torch.empty(N, geo.L, 2, device=dev)
        self.ref_all = torch.empty(T0, 2, device=dev)                     # sigmoid of the learned anchors
        self.toks, self.deltas = torch.empty(4, N, dtype=torch.int64, device=dev), torch.empty(4, N, device=dev)
        self.unfinished, self.step_t = torch.empty(N, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        self.out_logits = torch.zeros(N, max_len, model.num_classes, device=dev)
        self.out_coords, self.out_hs = torch.zeros(N, max_len, 2, device=dev), torch.zeros(N, max_len, 256, device=dev)
        self.alive = torch.zeros(max_len, dtype=torch.int32, device=dev)  # [i] = sequences still unfinished after step i
        # the reference's cache modules (kv_cache.py): K / V slabs (N, seq_len, 256) written in place at row `step`
        # (here: post-projection rows), VCache = the per-layer MSDA value projection of the image memory
        nhead = model.transformer.nhead
        self.kv = [KVCache(N, model.seq_len, 256, torch.float32).to(dev) for _ in dec.layers]
        self.vc = [VCache(N, geo.S, nhead, 256 // nhead, torch.float32).to(dev) for _ in dec.layers]
        self.caches = [{"k": kv.k_cache, "v": kv.v_cache, "value": vc.v_cache.view(N, geo.S, 256),
                        "sup_k": torch.empty(N, P, 256, device=dev) if P else None,
                        "sup_v": torch.empty(N, P, 256, device=dev) if P else None,
                        "sup_kpm": torch.empty(N, P, dtype=torch.uint8, device=dev) if (P and has_mask) else None}
                       for kv, vc in zip(self.kv, self.vc)]
        if tier != "per_op":
            self.ws = alloc_decode_workspace(N, len(dec.layers), geo.L, dev, geo.L * dec.layers[0].cross_attn.n_points)
            # layer-0 tables (its reference points are the learned anchors, the same for every image): query position
            # embedding per step, the (N, 2) reference rows the tail kernel refines and their level-scaled points
            self.qpos0, self.ref0 = torch.empty(T0, 256, device=dev), torch.empty(max_len, N, 2, device=dev)
            self.refin0 = torch.empty(max_len, N, geo.L, 2, device=dev)

    def begin_call(self, model):
        """Counts the call.  Captured steps and the whole-step descriptor hold raw weight pointers: if the parameters were
        re-homed since (model.to(), arena creation, load into new storage) or, in a fused tier, the folded weights were rebuilt
        (they follow every optimizer step / weight load), graphs, pool, descriptor and call count are dropped together."""
        key = tuple(p.data_ptr() for p in list(model.transformer.decoder.parameters())[:4]) + (model.query_embed.weight.data_ptr(),)
        if self.tier != "per_op":
            model._decode_weights.get()
            key = key + (model._decode_weights.key,)
        if self.weights_at != key:
            self.graphs, self.pool, self.plan, self.calls, self.weights_at = {}, None, None, 0, key
        self.calls += 1


def prepare(st, model, enc, support, smask):
    """Per-call tables: value / support K,V projections into the caches, anchors, first tokens, layer-0 tables."""
    dec, tok, N, P, geo, max_len = model.transformer.decoder, model.tokenizer, st.N, st.P, st.geo, st.max_len
    for layer, kv, vc in zip(dec.layers, st.kv, st.vc):      # the modules the reference's _setup_caches installs
        layer.kv_cache, layer.cross_attn.cache = kv, vc
    for layer, c in zip(dec.layers, st.caches):
        c["value"].copy_(layer.cross_attn.project_value(enc["memory"], enc["pad_rows"]))
        if P:
            ca = layer.support_attn
            s2 = support.contiguous().view(N * P, 256)
            ops.gemm(s2, ca.in_proj_weight[256:], c["sup_k"], N * P, 256, 256, bias=ca.in_proj_bias[256:])
            ops.gemm(s2, ca.in_proj_weight[512:], c["sup_v"], N * P, 256, 256, bias=ca.in_proj_bias[512:])
            if c["sup_kpm"] is not None:
                c["sup_kpm"].copy_(smask.to(torch.uint8))
    st.vr.copy_(enc["valid_ratios"])
    st.ref_all.copy_(ops.sigmoid_fwd(model.query_embed.weight.detach().contiguous()))            # (seq_len, 2)
    st.toks.fill_(tok.bos)
    st.deltas.copy_(torch.tensor([0.0, 1.0, 0.0, 1.0], device=st.deltas.device).view(4, 1).expand(4, N))
    st.unfinished.fill_(1)
    if st.tier == "per_op":
        return
    T0, qp0 = st.qpos0.shape[0], torch.empty_like(st.qpos0)
    ops.gemm(ops.query_sine_fwd(st.ref_all), dec.pos_trans.weight, qp0, T0, 256, 256, bias=dec.pos_trans.bias)
    qp0, _, _, _ = ops.add_layernorm_fwd(qp0, None, dec.pos_trans_norm.weight, dec.pos_trans_norm.bias)
    st.qpos0.copy_(qp0)
    st.ref0.copy_(st.ref_all[:max_len, None, :].expand(max_len, N, 2))
    st.refin0.copy_(ops.ref_scale_fwd(st.ref0.view(-1, 2), st.vr.repeat(max_len, 1, 1).contiguous(), 1, geo.L).view(max_len, N, geo.L, 2))
    ops.token_embed_fwd_into(dec.token_embed.weight, st.toks, st.deltas, st.ws["emb"])
    st.alive.zero_()
    if st.tier == "whole" and st.plan is None:
        st.plan = decode_plan(dec, model._decode_weights.layers, st.caches, st.ws["emb"], st.vr, geo, N, model.seq_len)


def make_step(st, model):
    """step(i, toks_i, deltas_i) of the state's tier: runs step i on the given input tokens (the state's own, or a teacher
    stream's), writes slot i of the outputs and, when fed the state's own tokens, advances them and `alive[i]`."""
    dec, tok, N, geo, toks, deltas, unfinished = model.transformer.decoder, model.tokenizer, st.N, st.geo, st.toks, st.deltas, st.unfinished
    out_logits, out_coords, out_hs, alive = st.out_logits, st.out_coords, st.out_hs, st.alive
    if st.tier == "per_op":
        def step(i, toks_i, deltas_i):
            ref_i = st.ref_all[i].view(1, 1, 2).expand(N, 1, 2).contiguous()
            hs, ref, cls = dec.decode_step(toks_i, deltas_i, ref_i, geo, st.vr, i, st.caches)
            out_logits[:, i] = cls; out_coords[:, i] = ref.view(N, 2); out_hs[:, i] = hs.view(N, 256)
            st.step_t.fill_(i)
            ops.decode_next_tokens(cls, ref.view(N, 2), unfinished, toks, deltas, st.step_t, N, tok.num_bins, MIN_LEN,
                                   tok.eos, tok.sep, tok.pad)
            alive[i] = unfinished.sum()
        return step
    emb, qpos0, refin0, ref0, table, dw = st.ws["emb"], st.qpos0, st.refin0, st.ref0, dec.token_embed.weight, model._decode_weights.layers
    if st.tier == "whole":
        launch = lambda i: st.plan.launch(i, qpos0[i], refin0[i], ref0[i], out_logits[:, i], out_coords[:, i], out_hs[:, i])
    else:
        launch = lambda i: decode_step_fused(dec, dw, st.ws, st.caches, geo, st.vr, i, qpos0[i], refin0[i], ref0[i], out_logits,
                                             out_coords, out_hs)

    def step(i, toks_i, deltas_i):
        if toks_i is not toks:                       # teacher forcing: the step's input tokens come from the stream
            ops.token_embed_fwd_into(table, toks_i, deltas_i, emb)
        launch(i)
        if toks_i is toks:
            ops.decode_advance(out_logits[:, i], out_coords[:, i], unfinished, toks, deltas, i, N, tok.num_bins, MIN_LEN,
                               tok.eos, tok.sep, tok.pad, table=table, embed_out=emb, alive_out=alive[i:i + 1])
    return step


def run_steps(st, step, teacher_stream, use_graphs, sync_every):
    """Runs steps 0.. until every sequence has finished (`alive` polled every `sync_every` steps) or `max_len`; teacher-forced,
    replayed (captured on first use) or eager.  Returns (steps run, length to trim the outputs to)."""
    i = 0
    while i < st.max_len:
        if teacher_stream is not None:
            t_i = torch.stack([teacher_stream[k][:, i] for k in ("seq11", "seq12", "seq21", "seq22")]).contiguous()
            d_i = torch.stack([teacher_stream[k][:, i] for k in ("delta_x1", "delta_x2", "delta_y1", "delta_y2")]).contiguous()
            step(i, t_i, d_i)
        elif use_graphs:
            g = st.graphs.get(i)
            if g is None:
                g = torch.cuda.CUDAGraph()
                if st.pool is None:
                    st.pool = torch.cuda.graph_pool_handle()
                with torch.cuda.graph(g, pool=st.pool, capture_error_mode="thread_local"):    # DataLoader pin-memory threads may call hipHostMalloc meanwhile
                    step(i, st.toks, st.deltas)
                st.graphs[i] = g
            g.replay()
        else:
            step(i, st.toks, st.deltas)
        i += 1
        if teacher_stream is None and (i % sync_every == 0 or i == st.max_len):
            done = (st.alive[:i].cpu() == 0).nonzero()
            if len(done):
                return i, min(int(done[0]) + 1, i)
    return i, i
