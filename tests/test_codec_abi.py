"""The v1.0 model's encoder / decoder convolutions on libgrr (csrc/codec_ops.hip, grr_conv1x1_cat2), host side:
the C ABI, its argument validation (before any launch: no GPU is needed), the plain-Python shape mirrors, the
NATIVE_CONVS switch's effect on the module surface, and the training graphs Dynamo captures with the switch on.
tests/test_gpu_codec.py runs the kernels.
"""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import irdu_amd
from irdu_amd import _native
from irdu_amd import graph_filter as GF
from irdu_amd import kernels as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["grr_conv3x3_embed", "grr_conv3x3_embed_bwd_w", "grr_conv3x3_embed_bwd_x", "grr_convt2x2s2",
                "grr_conv1x1_cat2"]
QUERIES = ["grr_conv3x3_embed_supported", "grr_conv3x3_embed_bwd_w_workspace_bytes", "grr_convt2x2s2_workspace_bytes",
           "grr_conv1x1_cat2_supported", "grr_conv1x1_cat2_workspace_bytes"]
INVALID_ARG, UNSUPPORTED = 1, 3


@pytest.fixture
def native_on():
    old = GF.NATIVE_CONVS
    irdu_amd.native_convs(True)
    yield
    irdu_amd.native_convs(old)


def test_entry_points_in_header_library_and_signatures():
    src = open(os.path.join(ROOT, "include", "grr.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(grr_[a-z0-9_]+)\s*\(", src))
    lib = _native.load()
    for name in ENTRY_POINTS + QUERIES:
        assert name in declared, f"{name} is not declared in include/grr.h"
        assert hasattr(lib, name), f"libgrr.so does not export {name}"
        assert name in _native.SIGNATURES, f"{name} has no ctypes signature"
    # the workspace queries: positive on a valid shape, 0 outside the range
    assert lib.grr_conv3x3_embed_bwd_w_workspace_bytes(2, 3, 48, 16, 20) >= 4 * 2 * 27 * 16 * 20
    assert lib.grr_conv3x3_embed_bwd_w_workspace_bytes(2, 5, 48, 16, 20) == 0
    assert lib.grr_convt2x2s2_workspace_bytes(2, 96, 48, 8, 10) >= 4 * (4 * 48 * 96 + 2 * 4 * 48 * 80)
    assert lib.grr_convt2x2s2_workspace_bytes(2, 0, 48, 8, 10) == 0
    assert lib.grr_conv1x1_cat2_workspace_bytes(48, 48, 48) == lib.grr_conv1x1_workspace_bytes(96, 48) > 0


def test_invalid_arguments_are_rejected_before_any_launch():
    lib = _native.load()
    one = 256   # a non-null, 256-byte aligned "pointer": validation fails before anything dereferences it
    cases = [
        ("grr_conv3x3_embed", (None, None, None, 1, 3, 48, 8, 8, None)),
        ("grr_conv3x3_embed", (one, one, 2 * one, 0, 3, 48, 8, 8, None)),
        ("grr_conv3x3_embed", (one, one, 2 * one, 1, 3, 48, 8, -1, None)),
        ("grr_conv3x3_embed", (one, 2 * one, one, 1, 3, 48, 8, 8, None)),          # out aliases x
        ("grr_conv3x3_embed_bwd_w", (None, None, None, None, 1, 3, 48, 8, 8, None)),
        ("grr_conv3x3_embed_bwd_w", (one, one, one, one, 1, 3, 0, 8, 8, None)),
        ("grr_conv3x3_embed_bwd_w", (one, one, one, one + 4, 1, 3, 48, 8, 8, None)),  # workspace misaligned
        ("grr_conv3x3_embed_bwd_x", (None, None, None, 1, 3, 48, 8, 8, None)),
        ("grr_conv3x3_embed_bwd_x", (one, one, 2 * one, 1, 3, 48, 0, 8, None)),
        ("grr_convt2x2s2", (None, None, None, None, 1, 96, 48, 8, 8, None)),
        ("grr_convt2x2s2", (one, one, 2 * one, one, 1, 96, 48, 8, 0, None)),
        ("grr_convt2x2s2", (one, one, 2 * one, one + 8, 1, 96, 48, 8, 8, None)),
        ("grr_conv1x1_cat2", (None, None, None, None, None, 1, 48, 48, 48, 64, None)),
        ("grr_conv1x1_cat2", (one, one, one, 2 * one, one, 1, 48, 0, 48, 64, None)),
        ("grr_conv1x1_cat2", (one, one, one, 2 * one, one, 1, 48, 48, 48, 0, None)),
    ]
    for name, args in cases:
        st = getattr(lib, name)(*args)
        assert st == INVALID_ARG, (name, args, st)
        assert lib.grr_last_error(), name
        assert name.encode() in lib.grr_last_error(), (name, lib.grr_last_error())
    # outside the supported range: a status of its own, also before any launch
    assert lib.grr_conv3x3_embed(one, one, 2 * one, 1, 5, 48, 8, 8, None) == UNSUPPORTED
    assert lib.grr_conv3x3_embed(one, one, 2 * one, 1, 3, 129, 8, 8, None) == UNSUPPORTED
    assert lib.grr_conv1x1_cat2(one, one, one, 2 * one, one, 1, 40, 24, 16, 64, None) == UNSUPPORTED
    assert b"Ka=40" in lib.grr_last_error()
    with pytest.raises(_native.GrrError):
        _native.call("grr_convt2x2s2", None, None, None, None, 1, 96, 48, 8, 8, None)


def test_python_mirrors_agree_with_the_library():
    lib = _native.load()
    # C4: 3 -> 48 embedding; dims 48/64/96/128 at 512 x 512 patches
    for cin, m in [(3, 48), (1, 1), (4, 128), (5, 48), (3, 129), (0, 48), (3, 0), (4, 64)]:
        assert K.conv3x3_embed_ok(cin, m) == bool(lib.grr_conv3x3_embed_supported(cin, m)), (cin, m)
    assert not K.conv3x3_embed_ok(5, 48) and not K.conv3x3_embed_ok(3, 129) and K.conv3x3_embed_ok(3, 48)
    for ka, kb, m, p in [(48, 48, 48, 512 * 512), (64, 64, 64, 256 * 256), (96, 96, 96, 128 * 128), (40, 24, 16, 64),
                         (16, 1, 1, 1), (0, 16, 16, 64), (48, 0, 48, 64), (4080, 32, 8, 64), (48, 48, 48, 1 << 24),
                         (192, 192, 192, 16), (8, 8, 8, 64), (48, 48, 0, 64), (48, 48, 48, 0)]:
        assert K.conv1x1_cat2_ok(ka, kb, m, p) == bool(lib.grr_conv1x1_cat2_supported(ka, kb, m, p)), (ka, kb, m, p)
    assert not K.conv1x1_cat2_ok(40, 24, 16, 64) and K.conv1x1_cat2_ok(48, 48, 48, 512 * 512)
    # C4 up-samplings: 128 -> 96 at 64^2, 96 -> 64 at 128^2, 64 -> 48 at 256^2 (batch 32)
    for k, m, h, w in [(128, 96, 64, 64), (96, 64, 128, 128), (64, 48, 256, 256), (0, 48, 8, 8), (4097, 48, 8, 8),
                       (8, 5, 1, 1), (8, 0, 4, 4), (8, 8, 0, 4), (8, 8, 16384, 16384)]:
        ok = lib.grr_convt2x2s2_workspace_bytes(32, k, m, h, w) > 0 and h * w * 16 < (1 << 31)
        assert K.convt2x2s2_ok(k, m, h, w) == ok, (k, m, h, w)


def test_wrappers_check_shapes_before_the_kernel():
    x, w = torch.zeros(1, 3, 4, 4), torch.zeros(8, 3, 3, 3)
    with pytest.raises(RuntimeError, match="GPU"):
        K.conv3x3_embed(x, w)
    with pytest.raises(RuntimeError, match="GPU"):
        K.convt2x2s2(torch.zeros(1, 8, 2, 2), torch.zeros(8, 4, 2, 2))
    with pytest.raises(RuntimeError, match="GPU"):
        K.conv1x1_cat2(torch.zeros(1, 16, 2, 2), torch.zeros(1, 16, 2, 2), torch.zeros(4, 32, 1, 1))


def _small_abstract(stages=3):
    torch.manual_seed(0)
    return irdu_amd.AbtractMultiScaleGraphFilter(
        3, 3, dims=[8, 16, 16, 32], hidden_dims=[16, 32, 32, 64], nsubnets=[1, 1, 1, 1], ngraphs=[2, 4, 4, 8],
        num_blocks=[1, 1, 1, 1], num_blocks_out=1, n_cgd_iters=stages)


def test_state_dict_keys_do_not_depend_on_the_switch(native_on):
    on = _small_abstract().state_dict()
    irdu_amd.native_convs(False)
    off = _small_abstract().state_dict()
    assert list(on) == list(off)
    assert all(on[k].shape == off[k].shape for k in on)


def test_switch_default_and_setter():
    assert os.environ.get("GRR_NATIVE_CONVS", "0") == ("1" if GF.NATIVE_CONVS else "0")
    old = GF.NATIVE_CONVS
    irdu_amd.native_convs(True)
    assert GF.NATIVE_CONVS is True
    irdu_amd.native_convs(old)
    assert GF.NATIVE_CONVS is old


def _record():
    from functorch.compile import make_boxed_func
    from torch._dynamo.backends.common import aot_autograd
    graphs = {"fw": [], "bw": []}

    def compiler(kind):
        def fn(gm, example_inputs):
            graphs[kind].append(gm)
            out_node = next(n for n in gm.graph.nodes if n.op == "output")
            vals = [a.meta.get("val") if isinstance(a, torch.fx.Node) else None for a in out_node.args[0]]

            def run(*args):
                return [None if v is None else torch.zeros(v.shape, dtype=v.dtype) for v in vals]
            return make_boxed_func(run)
        return fn

    return aot_autograd(fw_compiler=compiler("fw"), bw_compiler=compiler("bw")), graphs


def _targets(gms):
    seen = {}
    for gm in gms:
        for n in gm.graph.nodes:
            if n.op == "call_function":
                seen[str(n.target)] = seen.get(str(n.target), 0) + 1
    return seen


def test_compiled_training_graphs_hold_the_codec_ops(native_on):
    """Graphs only (the recording backend runs nothing): with the switch on, the captured training step of a
    small v1.0 model holds the embedding, the three up-samplings and the three combines as opaque irdu:: nodes,
    forward and reverse, and no aten convolution."""
    torch._dynamo.reset()
    backend, graphs = _record()
    m = _small_abstract().train()
    cm = torch.compile(m, backend=backend)
    x, c = torch.rand(2, 3, 32, 32), torch.rand(2, 3, 32, 32)
    F.l1_loss(cm(x), c).backward()
    fw, bw = _targets(graphs["fw"]), _targets(graphs["bw"])
    assert fw.get("irdu.conv3x3_embed_train.default") == 1, fw
    assert fw.get("irdu.convt2x2s2_train.default") == 3, fw
    assert fw.get("irdu.conv1x1_cat2_train.default") == 3, fw
    for op in ("conv3x3_embed_train", "convt2x2s2_train", "conv1x1_cat2_train"):
        assert f"irdu.{op}_backward.default" in bw, (op, bw)
    # the filter blocks' feature convolutions (8 + 4) plus linear_output and the three down-samplings
    assert fw.get("irdu.conv1x1_train.default") == 9 and fw.get("irdu.conv2x2s2_train.default") == 7, fw
    for name in ("aten.convolution", "aten.convolution_backward", "aten.mm", "aten.addmm", "aten.bmm"):
        assert not any(k.startswith(name) for k in list(fw) + list(bw)), name
    for p in m.parameters():
        assert p.grad is not None
    torch._dynamo.reset()
