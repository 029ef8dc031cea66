"""CPU checks of `--dilation` (the DC5 trunk of the reference's `models/backbone.py:72-83`: torchvision ResNet-50 with
`replace_stride_with_dilation=[False, False, True]` and the last stride halved): the product constructs with the same
state_dict as the undilated model, and the conv dilation field of the GEMM descriptor (`cape_gemm_desc.cDil`, appended under
ABI 11) is laid out and checked on the host as include/cape_hip.h says.  No device is involved."""
import ctypes

import pytest

import cape_amd  # noqa: F401
from cape_amd.hip import lib
from tests.helpers import build_product


@pytest.fixture(scope="module")
def models():
    _, _, plain, _ = build_product(device="cpu")
    _, _, dilated, _ = build_product(extra=("--dilation",), device="cpu")
    return plain, dilated


def test_dilated_product_constructs_with_the_same_state_dict(models):
    plain, dilated = models
    assert dilated.base_model.backbone.strides == [8, 16, 16]
    assert plain.base_model.backbone.strides == [8, 16, 32]
    sp, sd = plain.state_dict(), dilated.state_dict()
    assert list(sd.keys()) == list(sp.keys())
    for k in sp:
        assert tuple(sd[k].shape) == tuple(sp[k].shape), k
    count = lambda m, train: sum(p.numel() for p in m.parameters() if (p.requires_grad or not train))
    assert count(dilated, False) == count(plain, False) == 48247476
    assert count(dilated, True) == count(plain, True) == 47973876


def test_dilated_trunk_is_torchvisions_dc5(models):
    """torchvision `_make_layer(dilate=True)`: layer4's first block is stride 1 everywhere at the PREVIOUS dilation (1), its
    projection shortcut a 1x1 at stride 1; the second and third blocks use dilation 2 and padding 2.  Nothing before layer4 moves."""
    plain, dilated = models
    body, ref = dilated.base_model.backbone[0].body, plain.base_model.backbone[0].body
    l4 = body.layer4
    assert [(b.stride, b.dilation, b.conv2.stride, b.conv2.padding, b.conv2.dilation) for b in l4] == \
        [(1, 1, 1, 1, 1), (1, 2, 1, 2, 2), (1, 2, 1, 2, 2)]
    assert l4[0].downsample[0].stride == 1 and l4[0].downsample[0].kernel_size == 1
    assert [(b.stride, b.dilation) for b in ref.layer4] == [(2, 1), (1, 1), (1, 1)]
    for name in ("layer1", "layer2", "layer3"):
        assert [(b.stride, b.dilation, b.conv2.padding) for b in getattr(body, name)] == \
            [(b.stride, b.dilation, b.conv2.padding) for b in getattr(ref, name)]


def test_single_level_backbone_stride():
    from cape_amd.models.backbone import Backbone
    assert Backbone("resnet50", True, False, True).strides == [16]
    assert Backbone("resnet50", True, False, False).strides == [32]


def test_gemm_desc_dilation_field_layout():
    """`cDil` is the last field, fills the tail padding of the ABI-11 struct (the size every caller was compiled against does not
    change) and is zero in a zero-initialised descriptor."""
    names = [f[0] for f in lib.GemmDesc._fields_]
    assert names[-1] == "cDil" and names[-2] == "cTapWS"
    assert lib.GemmDesc.cDil.offset == lib.GemmDesc.cTapWS.offset + 4
    assert lib.GemmDesc.cDil.offset + 4 == ctypes.sizeof(lib.GemmDesc)
    assert lib.GemmDesc().cDil == 0


def test_bad_dilation_is_rejected_on_the_host():
    raw = lib.raw()
    d = lib.GemmDesc()
    d.cDil = -1
    assert raw.cape_gemm_f32(ctypes.byref(d), None) != 0 and "dilation" in lib.last_error()
    d.a_mode, d.b_mode = 1, 3                                # (the grouped launch takes the weight-gradient modes only)
    assert raw.cape_gemm_group_f32(ctypes.byref(d), 1, 64, None) != 0 and "dilation" in lib.last_error()
    # a tap sub-lattice (the stride-2 data gradient's parity classes) is worked out for undilated taps
    d = lib.GemmDesc()
    d.a_mode, d.b_mode, d.cStride, d.cKH, d.cKW, d.cKHp, d.cKWp, d.cDil = 3, 2, 1, 2, 2, 3, 3, 2
    assert raw.cape_gemm_f32(ctypes.byref(d), None) != 0 and "dilation" in lib.last_error()
    d.a_mode, d.b_mode = 1, 3
    assert raw.cape_gemm_group_f32(ctypes.byref(d), 1, 64, None) != 0 and "dilation" in lib.last_error()
    # 0 means 1: an empty product of a zero-initialised descriptor is still accepted
    assert raw.cape_gemm_f32(ctypes.byref(lib.GemmDesc()), None) == 0
