"""The ViT-Adapter's interaction blocks on the CPU: state-dict fidelity, fp64 parity with the reference's fixtures
(tests/golden/make_golden_adapter.py) with the CPU oracle standing in for the HIP op, the cached deform inputs, and
the host side of the C ABI of the encoder's sampling plan.  The same blocks run on the GPU with the real op and the
fused front end in test_vit_adapter_gpu.py."""
import ast
import ctypes
import glob
import os
import re
from collections import namedtuple

import numpy as np
import pytest
import torch

from helpers import GOLDEN
from oracle.msda_oracle import OracleMSDAFunction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mmfs_msda.h")
Hidden = namedtuple("Hidden", "last_hidden_state")


def load_fixture(name):
    """A fixture and its parts (``<name>.npz``, ``<name>.p<k>.npz``) as one dictionary."""
    z = {}
    for path in [os.path.join(GOLDEN, name + ".npz")] + sorted(glob.glob(os.path.join(GOLDEN, name + ".p*.npz"))):
        z.update(np.load(path, allow_pickle=False))
    return z


def T(a, dtype=torch.float64, device="cpu"):
    t = torch.from_numpy(np.asarray(a)).to(device)
    return t.to(dtype) if t.is_floating_point() and dtype is not None else t


def rel(a, b):
    a = a.detach().double().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, np.float64)
    b = np.asarray(b, np.float64).reshape(a.shape)
    return float(np.abs(a - b).max() / max(float(np.abs(b).max()), 1e-300))


def deform_of(z, which, dtype=torch.float64, device="cpu"):
    return [T(z[which + ".reference_points"], dtype, device), T(z[which + ".spatial_shapes"], None, device),
            T(z[which + ".level_start_index"], None, device)]


def build(name, z, dtype=torch.float64, device="cpu", **over):
    from mmfs_amd.blocks import Extractor, Injector, InteractionBlockWithCls
    cls = {"adapter_injector": Injector, "adapter_extractor": Extractor,
           "adapter_interaction_cls": InteractionBlockWithCls}[name]
    m = cls(**dict(ast.literal_eval(str(z["cfg"])), **over))
    sd = {k[len("param."):]: T(v, torch.float64) for k, v in z.items() if k.startswith("param.")}
    return m, sd


def call(name, m, z, xs, dtype=torch.float64, device="cpu"):
    """The fixture's call of block ``name`` -> tuple of outputs in the fixture's order."""
    hw = int(z["image_hw"][0]) // 16
    if name == "adapter_injector":
        return (m(xs["query"], *deform_of(z, "di1", dtype, device)[:1], xs["feat"], *deform_of(z, "di1", dtype, device)[1:]),)
    if name == "adapter_extractor":
        d = deform_of(z, "di2", dtype, device)
        return (m(xs["query"], d[0], xs["feat"], d[1], d[2], hw, hw),)
    Wb = T(z["extra.Wb"], dtype, device)
    blocks = lambda t: Hidden(t + torch.tanh(t @ Wb))     # noqa: E731
    return m(xs["x"], xs["c"], xs["cls"], blocks, deform_of(z, "di1", dtype, device), deform_of(z, "di2", dtype, device), hw, hw)


OUTS = {"adapter_injector": ("out",), "adapter_extractor": ("out",), "adapter_interaction_cls": ("x", "c", "cls")}
CASES = sorted(OUTS)


@pytest.fixture()
def oracle_op(monkeypatch):
    import mmfs_amd.modules.ms_deform_attn as m2
    monkeypatch.setattr(m2, "MSDeformAttnFunction", OracleMSDAFunction)


@pytest.mark.parametrize("name", CASES)
def test_state_dict_is_the_references(name):
    z = load_fixture(name)
    m, sd = build(name, z)
    own = m.state_dict()
    assert set(own) == set(sd)
    for k, v in sd.items():
        assert tuple(own[k].shape) == tuple(v.shape), k
    m.double().load_state_dict(sd, strict=True)
    for mod in m.modules():
        if type(mod).__name__ == "MSDeformAttn":
            assert mod.fused_front_end is True


def run_block(name, z, **over):
    m, sd = build(name, z, **over)
    m = m.double()
    m.load_state_dict(sd, strict=True)
    m.train()                                         # (checkpointing and drop-path are training-mode behaviour)
    xs = {k[len("in."):]: T(v).requires_grad_(True) for k, v in z.items() if k.startswith("in.")}
    outs = call(name, m, z, xs)
    torch.autograd.backward(list(outs), [T(z["grad_out." + n]) for n in OUTS[name]])
    return m, xs, outs


@pytest.mark.parametrize("with_cp", [False, True])
@pytest.mark.parametrize("name", CASES)
def test_blocks_match_the_reference_in_fp64(name, with_cp, oracle_op):
    """Outputs, input gradients and every parameter gradient within 1e-9 of the largest reference entry."""
    z = load_fixture(name)
    m, xs, outs = run_block(name, z, with_cp=with_cp)
    for n, o in zip(OUTS[name], outs):
        assert rel(o, z["out." + n]) <= 1e-9, n
    for k, x in xs.items():
        assert rel(x.grad, z["grad_in." + k]) <= 1e-9, k
    params = dict(m.named_parameters())
    assert {"grad." + k for k in params} == {k for k in z if k.startswith("grad.")}
    for k, p in params.items():
        assert rel(p.grad, z["grad." + k]) <= 1e-9, k


def test_block_without_cls_token_matches_the_one_with(oracle_op):
    """InteractionBlock on the weights of InteractionBlockWithCls: with ``blocks`` a list of per-token layers and
    no class token, x and c are what the cls block gives for a ``blocks`` that acts per token."""
    from mmfs_amd.blocks import InteractionBlock
    name = "adapter_interaction_cls"
    z = load_fixture(name)
    m_cls, sd = build(name, z)
    m_cls.double().load_state_dict(sd, strict=True)
    m = InteractionBlock(**ast.literal_eval(str(z["cfg"]))).double()
    m.load_state_dict(sd, strict=True)
    xs = {k[len("in."):]: T(v) for k, v in z.items() if k.startswith("in.")}
    Wb = T(z["extra.Wb"])
    hw = int(z["image_hw"][0]) // 16
    d1, d2 = deform_of(z, "di1"), deform_of(z, "di2")
    with torch.no_grad():
        x, c = m(xs["x"], xs["c"], [lambda t, H, W: t + torch.tanh(t @ Wb)], d1, d2, hw, hw)
        x2, c2, _ = m_cls(xs["x"], xs["c"], xs["cls"], lambda t: Hidden(t + torch.tanh(t @ Wb)), d1, d2, hw, hw)
    assert rel(x, z["out.x"]) <= 1e-9 and rel(c, z["out.c"]) <= 1e-9
    # (not bit for bit: the stand-in's matrix product runs on 64 and on 65 token rows, and a BLAS may block the two
    # differently -- fp64 sums of 128 terms in another order, <= 128 * 2^-53 each, a few of them chained)
    assert rel(x, x2.numpy()) <= 1e-12 and rel(c, c2.numpy()) <= 1e-12


def test_deform_inputs_are_cached_and_equal_the_references():
    from mmfs_amd.blocks import deform_inputs, get_reference_points
    z = load_fixture("adapter_injector")
    h, w = (int(v) for v in z["image_hw"])
    a1, a2 = deform_inputs(torch.zeros(2, 3, h, w))
    b1, b2 = deform_inputs(torch.zeros(5, 3, h, w))
    for a, b in zip(a1 + a2, b1 + b2):
        assert a is b
    for got, which in ((a1, "di1"), (a2, "di2")):
        # (pixel centres in fp32: linspace's start + i * step and the division round once each, and a CPU's vector width
        # may place those roundings differently from the machine the fixture was made on: one ulp of 1.0)
        assert got[0].dtype == torch.float32 and got[0].shape == z[which + ".reference_points"].shape
        assert float((got[0] - T(z[which + ".reference_points"], None)).abs().max()) <= 2.0 ** -23
        assert got[1].dtype == torch.int64 and torch.equal(got[1], T(z[which + ".spatial_shapes"], None))
        assert got[2].dtype == torch.int64 and torch.equal(got[2], T(z[which + ".level_start_index"], None))
        assert got[1].is_contiguous() and got[2].is_contiguous()
    c1, _ = deform_inputs(torch.zeros(1, 3, h, 2 * w))       # another image size: other tensors
    assert c1[0] is not a1[0] and c1[0].shape[1] == (h // 16) * (2 * w // 16)
    assert get_reference_points([(h // 16, w // 16)], "cpu") is a1[0]


def test_drop_path_is_stochastic_depth_without_timm():
    import sys
    from mmfs_amd.blocks import Extractor
    from mmfs_amd.blocks.vit_adapter import DropPath
    assert "timm" not in sys.modules
    e = Extractor(dim=32, num_heads=2, n_points=2, deform_ratio=0.5, drop_path=0.25)
    assert isinstance(e.drop_path, DropPath)
    assert isinstance(Extractor(dim=32, num_heads=2, n_points=2).drop_path, torch.nn.Identity)
    dp = DropPath(0.25)
    x = torch.ones(4000, 3, 2)
    dp.eval()
    assert dp(x) is x
    dp.train()
    torch.manual_seed(0)
    y = dp(x)
    per_sample = y[:, 0, 0]
    assert set(per_sample.unique().tolist()) == {0.0, float(torch.tensor(1.0) / 0.75)}          # dropped whole, or kept and rescaled
    assert torch.equal(y, per_sample[:, None, None].expand_as(y))
    assert abs(float((per_sample == 0).float().mean()) - 0.25) < 0.03
    assert abs(float(y.mean()) - 1.0) < 0.05


def test_module_switch_is_off_by_default_and_leaves_the_state_dict_alone():
    from mmfs_amd.modules import MSDeformAttn
    m = MSDeformAttn(d_model=32, n_levels=2, n_heads=2, n_points=2)
    assert MSDeformAttn.fused_front_end is False and m.fused_front_end is False
    keys = set(m.state_dict())
    assert keys == {p + s for p in ("sampling_offsets.", "attention_weights.", "value_proj.", "output_proj.")
                    for s in ("weight", "bias")}
    m.fused_front_end = True
    assert set(m.state_dict()) == keys
    # on the CPU the switch changes nothing: the framework-op statement runs
    q, f = torch.randn(1, 3, 32), torch.randn(1, 5, 32)
    ref = torch.rand(1, 3, 2, 2)
    sh, st = torch.tensor([[2, 2], [1, 1]]), torch.tensor([0, 4])
    import mmfs_amd.modules.ms_deform_attn as mod
    real = mod.MSDeformAttnFunction
    try:
        mod.MSDeformAttnFunction = OracleMSDAFunction
        a = m.double()(q.double(), ref.double(), f.double(), sh, st)
        m.fused_front_end = False
        b = m(q.double(), ref.double(), f.double(), sh, st)
    finally:
        mod.MSDeformAttnFunction = real
    assert torch.equal(a, b)


# ------------------------------------------------------------------ C ABI, host side
from helpers import bound_library as _lib  # noqa: E402


def test_new_symbols_are_declared_and_exported_at_abi_14():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = _lib()
    for n in ("mmfs_deform_plan_supported", "mmfs_deform_plan_forward", "mmfs_deform_plan_backward",
              "mmfs_deform_sample_forward"):
        assert re.search(r"\b" + n + r"\s*\(", text), n
        assert hasattr(lib, n), n
    assert lib.mmfs_msda_abi_version() == 14
    assert int(re.search(r"#define\s+MMFS_MSDA_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1)) == 14


def test_supported_query():
    f = _lib().mmfs_deform_plan_supported
    for dt in (0, 1, 2):
        for P in (2, 4, 8):
            for L in (1, 2, 3, 8):
                for R in (2, 4):
                    assert f(dt, L, P, R, 0) == 1
    assert f(2, 3, 4, 2, 32) == 3 and f(2, 1, 4, 2, 16) == 3 and f(0, 1, 4, 2, 64) == 3 and f(1, 2, 2, 4, 16) == 3
    assert f(2, 3, 4, 2, 24) == 1 and f(0, 3, 4, 2, 4) == 1        # rows the gather's 16-byte lanes cannot take
    assert f(3, 3, 4, 2, 0) == 0 and f(9, 3, 4, 2, 0) == 0         # fp64 / unknown dtype
    assert f(2, 9, 4, 2, 0) == 0 and f(2, 0, 4, 2, 0) == 0 and f(2, 3, 3, 2, 0) == 0 and f(2, 3, 16, 2, 0) == 0
    assert f(2, 3, 4, 3, 0) == 0


def test_argument_errors_and_empty_problems_return_before_any_launch():
    lib = _lib()
    fake = ctypes.c_void_p(4096)                       # aligned, never dereferenced on these paths
    #        N  Lq  H  L  P  Nr Lref R
    dims = [2, 16, 4, 3, 4, 1, 1, 2]

    def fwd(dt, dims, ptr=fake, ld=(0, 0)):
        return lib.mmfs_deform_plan_forward(dt, ptr, ptr, ld[0], ld[1], ptr, ptr, ptr, ptr, *dims, None)

    def bwd(dt, dims, ptr=fake, ld=(0, 0)):
        return lib.mmfs_deform_plan_backward(dt, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ld[0], ld[1], *dims, None)

    def smp(dt, dims, S=336, D=32, ptr=fake, ld=(0, 0)):
        N, Lq, H, L, P, Nr, Lref, R = dims
        return lib.mmfs_deform_sample_forward(dt, ptr, ptr, ptr, ptr, ptr, ld[0], ld[1], ptr, ptr,
                                              N, S, Lq, H, D, L, P, Nr, Lref, R, None)

    def with_(i, v):
        return dims[:i] + [v] + dims[i + 1:]

    for f in (fwd, bwd, smp):
        assert f(9, dims) == -1 and f(3, dims) == -1                   # dtype (fp64 is not a storage type here)
        assert f(2, with_(0, -1)) == -2 and f(2, with_(1, -1)) == -2   # negative dims
        assert f(2, with_(2, 0)) == -2 and f(2, with_(3, 0)) == -2
        assert f(2, with_(5, 3)) == -2                                 # Nr not in {1, N}
        assert f(2, with_(6, 2)) == -2                                 # Lref not in {1, L}
        assert f(2, with_(7, 3)) == -2                                 # R not in {2, 4}
        assert f(2, with_(4, 3)) == -5 and f(2, with_(4, 16)) == -5    # P outside {2, 4, 8}
        assert f(2, with_(3, 9)) == -5                                 # L > 8
        assert f(2, dims, ptr=None) == -3                              # NULL tensors of a non-empty problem
        assert f(2, with_(0, 0), ptr=None) == 0                        # empty batch
        assert f(2, with_(1, 0), ptr=None) == 0                        # no queries
        assert f(2, dims, ld=(8, 0)) == -2                             # leading dimension below the packed row
        assert f(2, dims, ld=(4 * 3 * 4 * 2 + 1, 0)) == -4             # rows the vector accesses cannot take
    assert smp(2, dims, D=24) == -5 and smp(0, dims, D=4) == -5        # head rows the gather cannot take: plan + op
    assert smp(2, dims, D=-1) == -2 and smp(2, dims, S=-1) == -2
