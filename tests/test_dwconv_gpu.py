"""ConvFFN's depthwise convolution in the token layout on the GPU (csrc/msda_dwconv.hip).

1. forward and backward through the C ABI, every element against the fp64 evaluation on the same storage-rounded
   inputs under a derived bound, outputs allocated poisoned;  2. level seams, non-finite inputs, determinism, empty and
   unsupported problems;  3. ``DWConv`` / ``ConvFFN`` inside the blocks on the reference's fixtures, with a route
   counter, under checkpointing and under graph capture."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

import helpers
from helpers import STORAGE_T, STORAGE_U
from test_vit_adapter import OUTS, T, call, load_fixture, rel
from test_vit_adapter_gpu import gpu_block, worst

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
CODE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
ACT = {"none": 0, "gelu": 1}
K_ERF = 8       # see test_forward_and_backward_element_by_element

TABLES = {
    "adapter8": [(16, 16), (8, 8), (4, 4)],
    "adapter16": [(32, 32), (16, 16), (8, 8)],
    "nonsquare": [(12, 20), (6, 10), (3, 5)],
    "one": [(9, 11)],
    "degenerate": [(1, 1), (1, 7), (7, 1), (2, 2)],
    "eight": [(5, 3), (2, 4), (1, 1), (3, 3), (4, 2), (1, 5), (6, 1), (17, 2)],
}


def lib():
    from mmfs_amd.functions import dwconv_func
    return dwconv_func._lib


def stream():
    return torch.cuda.current_stream().cuda_stream


def host_table(maps):
    return (ctypes.c_int64 * (2 * len(maps)))(*[v for hw in maps for v in hw])


def images(t, maps):
    """[B, N, C] -> one [B, C, h, w] image per map"""
    B, _, C = t.shape
    out, lo = [], 0
    for h, w in maps:
        out.append(t[:, lo:lo + h * w].transpose(1, 2).reshape(B, C, h, w))
        lo += h * w
    return out


def tokens(imgs):
    return torch.cat([i.flatten(2).transpose(1, 2) for i in imgs], 1)


def conv64(t, w, maps, flip=False):
    """the depthwise 3x3 convolution (``flip``: its adjoint) of every map of t [B, N, C] with w [C, 1, 3, 3], fp64"""
    w = w.flip(2, 3) if flip else w
    return tokens([F.conv2d(i, w, None, 1, 1, 1, w.shape[0]) for i in images(t, maps)])


def wsum64(x, g, maps):
    """[C, 1, 3, 3]: sum over samples and pixels of x[p] g[p - d]"""
    C = x.shape[2]
    acc = torch.zeros(C, 3, 3, dtype=torch.float64, device=x.device)
    for xi, gi in zip(images(x, maps), images(g, maps)):
        h, w = gi.shape[2:]
        xp = F.pad(xi, (1, 1, 1, 1))
        for ky in range(3):
            for kx in range(3):
                acc[:, ky, kx] += (xp[:, :, ky:ky + h, kx:kx + w] * gi).sum((0, 2, 3))
    return acc.view(C, 1, 3, 3)


def gelu64(y):
    return 0.5 * y * (1.0 + torch.erf(y / math.sqrt(2.0)))


def gelu_grad64(y):
    return 0.5 * (1.0 + torch.erf(y / math.sqrt(2.0))) + y * torch.exp(-0.5 * y * y) / math.sqrt(2.0 * math.pi)


def chain_length(B, maps, C):
    """n of the grad_w / grad_b bounds, by the rule in the header comment of csrc/msda_dwconv.hip: a lane's strip of 16
    rows + the LDS tree over a workgroup's items + a reducer lane's rows + the reducer's tree of 16 + 2."""
    clb = 1
    while clb < min(C // 4, 256):
        clb *= 2
    ipb = 256 // clb
    groups = -(-B * sum(-(-h // 16) * w for h, w in maps) // ipb)
    return 16 + int(math.log2(ipb)) + -(-groups // 16) + 4 + 2


def make_case(dtype, B, maps, C, bias, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    N = sum(h * w for h, w in maps)
    x = torch.randn(B, N, C, device=DEV, generator=g).to(dtype)
    w = (torch.randn(C, 1, 3, 3, device=DEV, generator=g) * 0.4).to(dtype)
    b = torch.randn(C, device=DEV, generator=g).to(dtype) if bias else None
    ga = torch.randn(B, N, C, device=DEV, generator=g).to(dtype)
    return x, w, b, ga


def run_forward(dtype, x, w, b, maps, act, want_pre=True):
    B, N, C = x.shape
    out = torch.empty(B, N, C, device=DEV, dtype=dtype)
    pre = torch.empty(B, N, C, device=DEV, dtype=dtype) if want_pre and act == "gelu" else None
    rc = lib().mmfs_dwconv_tokens_forward(CODE[dtype], x.data_ptr(), w.data_ptr(), None if b is None else b.data_ptr(),
                                          out.data_ptr(), None if pre is None else pre.data_ptr(), host_table(maps),
                                          B, N, C, len(maps), ACT[act], stream())
    assert rc == 0, rc
    return out, pre


def run_backward(dtype, ga, x, pre, w, has_bias, maps, act):
    B, N, C = x.shape
    table = host_table(maps)
    nbytes = lib().mmfs_dwconv_tokens_backward_workspace_bytes(CODE[dtype], table, B, N, C, len(maps), ACT[act])
    assert nbytes > 0
    ws = torch.empty(nbytes, device=DEV, dtype=torch.uint8)
    gx, gw = torch.empty_like(x), torch.empty_like(w)
    gb = torch.empty(C, device=DEV, dtype=dtype) if has_bias else None
    rc = lib().mmfs_dwconv_tokens_backward(CODE[dtype], ga.data_ptr(), x.data_ptr(), None if pre is None else pre.data_ptr(),
                                           w.data_ptr(), gx.data_ptr(), gw.data_ptr(), None if gb is None else gb.data_ptr(),
                                           ws.data_ptr(), table, B, N, C, len(maps), ACT[act], stream())
    assert rc == 0, rc
    return gx, gw, gb


def check_case(dtype, act, B, maps, C, bias, seed, report):
    """One problem, forward and backward, every element of every output under its bound."""
    u, t = STORAGE_U[dtype], STORAGE_T[dtype]
    x, w, b, ga = make_case(dtype, B, maps, C, bias, seed)
    out, pre = run_forward(dtype, x, w, b, maps, act)
    x64, w64, ga64 = x.double(), w.double(), ga.double()
    b64 = b.double() if bias else torch.zeros(C, dtype=torch.float64, device=DEV)
    y_ref = conv64(x64, w64, maps) + b64
    S = conv64(x64.abs(), w64.abs(), maps) + b64.abs()
    y_t = pre if act == "gelu" else out
    res = {"y": worst(y_t, y_ref, u * y_ref.abs() + 2.0 ** -19 * S + t)}
    if act == "gelu":
        yk = pre.double()                                  # the kernel's own rounded pre-activation
        a_ref = gelu64(yk)
        res["a"] = worst(out, a_ref, u * a_ref.abs() + K_ERF * 2.0 ** -24 * yk.abs() + t)
        out2, _ = run_forward(dtype, x, w, b, maps, act, want_pre=False)
        assert torch.equal(out2, out), "the call without the pre-activation returns other bits"
        gy = ga64 * gelu_grad64(yk)
        dgelu = 2.0 ** -21
    else:
        gy, dgelu = ga64, 0.0
    gx, gw, gb = run_backward(dtype, ga, x, pre, w, bias, maps, act)
    n = chain_length(B, maps, C)
    gx_ref = conv64(gy, w64, maps, flip=True)
    res["grad_x"] = worst(gx, gx_ref, u * gx_ref.abs() + 2.0 ** -19 * conv64(gy.abs(), w64.abs(), maps, flip=True)
                          + dgelu * conv64(ga64.abs(), w64.abs(), maps, flip=True) + t)
    gw_ref = wsum64(x64, gy, maps)
    res["grad_w"] = worst(gw, gw_ref, u * gw_ref.abs() + n * 2.0 ** -24 * wsum64(x64.abs(), gy.abs(), maps)
                          + dgelu * wsum64(x64.abs(), ga64.abs(), maps) + t)
    if bias:
        gb_ref = gy.sum((0, 1))
        res["grad_b"] = worst(gb, gb_ref, u * gb_ref.abs() + n * 2.0 ** -24 * gy.abs().sum((0, 1))
                              + dgelu * ga64.abs().sum((0, 1)) + t)
    for k, v in res.items():
        report[k] = max(report.get(k, 0.0), v[0])
    bad = {k: v for k, v in res.items() if not v[0] <= 1.0}
    assert not bad, f"{dtype} act={act} B={B} maps={maps} C={C} bias={bias}: bound broken: {bad}"


@pytest.mark.parametrize("act", ["none", "gelu"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_forward_and_backward_element_by_element(dtype, act, monkeypatch):
    """Every element of y_T, a, grad_x, grad_w and grad_b against fp64 on the same storage-rounded inputs (u = the
    storage type's rounding, t its subnormal floor, S = |b| + sum |w x| over the window):
        |y - ref|      <= u |ref| + 2^-19 S + t                      (10 terms: at most 19 fp32 roundings, 19 * 2^-24 < 2^-19)
        |a - ref|      <= u |ref| + k 2^-24 |y_T| + t                (ref: fp64 GELU of the kernel's own y_T)
        |grad_x - ref| <= u |ref| + 2^-19 sum |w g_y| + 2^-21 sum |w| |g_a| + t
        |grad_w - ref| <= u |ref| + n 2^-24 sum |x g_y| + 2^-21 sum |x| |g_a| + t      (per tap; grad_b: x = 1)
    (the 2^-21 terms carry the error of gelu' and are absent for act = none).
    k = 8: the middle term of a's bound is the absolute error of erf near +-1 times |y| / 2 (for negative y, 1 + erf
    cancels), doubled for the two further roundings of the product.  ROCm's headers give erff as a call of the device
    library's __ocml_erf_f32 (__clang_hip_math.h) and state no accuracy for it, and ROCm installs no document that
    does; the figure used is the one the HIP programming guide's table of device math
    functions publishes for erff, a maximum error of 4 ulp: 4 * 2^-24 * |y| / 2, doubled, = 8 * 2^-24 |y|.
    n = the longest chain of sequential fp32 additions of the two-stage reduction + 2, from the rule in the kernel's
    header comment (chain_length).
    Outputs are allocated poisoned: an element no lane writes is NaN and fails.  No element is left out."""
    helpers.poison_allocations(monkeypatch)
    report, seed = {}, 0
    for bias in (True, False):
        for C in (8, 32, 72, 256):
            for name, maps in TABLES.items():
                for B in (1, 3):
                    seed += 1
                    check_case(dtype, act, B, maps, C, bias, seed, report)
    print(f"DWCONV-BOUNDS {str(dtype)[6:]} act={act} worst ratios " + " ".join(f"{k} {v:.3f}" for k, v in report.items()))


@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_batch_and_unsupported_width(dtype):
    from mmfs_amd.blocks import ConvFFN, DWConv
    from mmfs_amd.functions import DWConvTokensFunction, dwconv_func, dwconv_tokens_supported
    maps = ((8, 8), (4, 4), (2, 2))
    conv = torch.nn.Conv2d(32, 32, 3, 1, 1, groups=32).to(DEV, dtype)
    # B = 0: an empty result, nothing launched, and gradients of the right shapes
    x = torch.zeros(0, 84, 32, device=DEV, dtype=dtype, requires_grad=True)
    for act in ("none", "gelu"):
        out = DWConvTokensFunction.apply(x, conv.weight, conv.bias, maps, act)
        assert out.shape == (0, 84, 32) and out.dtype == dtype
        gx, gw, gb = torch.autograd.grad(out, [x, conv.weight, conv.bias], torch.zeros_like(out))
        assert gx.shape == x.shape and not gw.any() and not gb.any()
    # a width the 16-byte lanes cannot take: the query refuses it and the module returns the framework's result
    C = 12 if dtype != torch.float32 else 6
    odd = DWConv(C).to(DEV, dtype)
    xo = torch.randn(2, 84, C, device=DEV).to(dtype)
    assert not dwconv_tokens_supported(xo, odd.dwconv.weight, odd.dwconv.bias)
    assert lib().mmfs_dwconv_tokens_supported(CODE[dtype], C, 3, 0) == 0
    before = dict(dwconv_func.launches)
    got = odd(xo, 4, 4)
    odd.token_kernel = False
    assert torch.equal(got, odd(xo, 4, 4)) and dwconv_func.launches == before
    ffn = ConvFFN(16, C).to(DEV, dtype)
    xf = torch.randn(2, 84, 16, device=DEV).to(dtype)
    got = ffn(xf, 4, 4)
    ffn.dwconv.token_kernel = False
    assert torch.equal(got, ffn(xf, 4, 4)) and dwconv_func.launches == before
    # mixed dtypes and autocast take the framework statement too
    ok = DWConv(32).to(DEV, dtype)
    xs = torch.randn(2, 84, 32, device=DEV).to(dtype)
    assert dwconv_tokens_supported(xs, ok.dwconv.weight, ok.dwconv.bias)
    other = torch.float16 if dtype != torch.float16 else torch.bfloat16
    assert not dwconv_tokens_supported(xs.to(other), ok.dwconv.weight, ok.dwconv.bias)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert ok.tokens(xs, 4, 4, "none") is None
    assert ok.tokens(xs, 4, 4, "none") is not None


@pytest.mark.parametrize("act", ["none", "gelu"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_taps_never_cross_a_level_seam(dtype, act, monkeypatch):
    """Two inputs that differ only in the border rows of the NEIGHBOURING maps give the same bits in a map: in the
    packed layout the last row of one map is followed at once by the first row of the next."""
    helpers.poison_allocations(monkeypatch)
    maps = [(6, 5), (4, 7), (3, 3)]
    x, w, b, ga = make_case(dtype, 2, maps, 32, True, 11)
    x2, ga2 = x.clone(), ga.clone()
    g = torch.Generator(device=DEV).manual_seed(12)
    lo0, lo1, lo2 = 0, 30, 58
    for t2 in (x2, ga2):
        t2[:, lo1 - 5:lo1] = torch.randn(2, 5, 32, device=DEV, generator=g).to(dtype)        # last row of map 0
        t2[:, lo2:lo2 + 3] = torch.randn(2, 3, 32, device=DEV, generator=g).to(dtype)        # first row of map 2
    out, pre = run_forward(dtype, x, w, b, maps, act)
    out2, pre2 = run_forward(dtype, x2, w, b, maps, act)
    assert torch.equal(out[:, lo1:lo2], out2[:, lo1:lo2])
    assert not torch.equal(out[:, lo0:lo1], out2[:, lo0:lo1]) and not torch.equal(out[:, lo2:], out2[:, lo2:])
    # backward: grad_x of map 1 reads g_a / y_T of map 1 only (the pre-activation of map 1 is the same in both)
    if act == "gelu":
        assert torch.equal(pre[:, lo1:lo2], pre2[:, lo1:lo2])
    gx, _, _ = run_backward(dtype, ga, x, pre, w, True, maps, act)
    gx2, _, _ = run_backward(dtype, ga2, x2, pre2, w, True, maps, act)
    assert torch.equal(gx[:, lo1:lo2], gx2[:, lo1:lo2])


@pytest.mark.parametrize("act", ["none", "gelu"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_non_finite_inputs_reach_exactly_their_windows(dtype, act, monkeypatch):
    """One Inf and one NaN in x: the non-finite elements of y are those of the fp64 framework convolution (a skipped tap
    is never multiplied by 0), every other element stays within its bound."""
    helpers.poison_allocations(monkeypatch)
    u, t = STORAGE_U[dtype], STORAGE_T[dtype]
    maps = TABLES["adapter8"]
    x, w, b, _ = make_case(dtype, 2, maps, 32, True, 21)
    w = torch.where(w == 0, torch.ones_like(w), w)         # (an exactly zero weight times Inf would be NaN in both, but keep the sets sharp)
    x[0, 0, 3] = float("inf")                              # a corner of map 0
    x[1, 256 + 63, 5] = float("nan")                       # the last pixel of map 1, next to map 2 in memory
    out, pre = run_forward(dtype, x, w, b, maps, act)
    y = pre if act == "gelu" else out
    y_ref = conv64(x.double(), w.double(), maps) + b.double()
    bad_ref = ~torch.isfinite(y_ref)
    assert torch.equal(~torch.isfinite(y.double()), bad_ref)
    assert int(bad_ref.sum()) == 4 + 4
    xa = torch.where(torch.isfinite(x), x, torch.zeros_like(x)).double()
    S = conv64(xa.abs(), w.double().abs(), maps) + b.double().abs()
    bound = u * y_ref.abs() + 2.0 ** -19 * S + t
    fin = ~bad_ref
    err = (y.double() - y_ref).abs()
    assert bool((err[fin] <= bound[fin]).all())
    assert torch.equal(~torch.isfinite(out.double()), bad_ref)


@pytest.mark.parametrize("dtype", DTYPES)
def test_weight_and_bias_gradients_are_deterministic(dtype, monkeypatch):
    helpers.poison_allocations(monkeypatch)
    maps = TABLES["adapter16"]
    x, w, b, ga = make_case(dtype, 3, maps, 72, True, 31)
    _, pre = run_forward(dtype, x, w, b, maps, "gelu")
    first = run_backward(dtype, ga, x, pre, w, True, maps, "gelu")
    junk = torch.randn(1 << 20, device=DEV)                # (another allocation pattern between the calls)
    second = run_backward(dtype, ga, x, pre, w, True, maps, "gelu")
    del junk
    for a, c in zip(first, second):
        assert torch.isfinite(a).all() and torch.equal(a, c)


# ------------------------------------------------------------------ the blocks on the reference's fixtures
def block_step(name, z, on, with_cp=False):
    from mmfs_amd.blocks import DWConv
    from mmfs_amd.functions import dwconv_func
    m = gpu_block(name, z, torch.float32, with_cp=with_cp).train()
    n_ffn = 0
    for mod in m.modules():
        if isinstance(mod, DWConv):
            mod.token_kernel = on
            n_ffn += 1
    xs = {k[len("in."):]: T(v, torch.float32, DEV).requires_grad_(True) for k, v in z.items() if k.startswith("in.")}
    before = dict(dwconv_func.launches)
    outs = call(name, m, z, xs, torch.float32, DEV)
    fwd = dwconv_func.launches["forward"] - before["forward"]
    torch.autograd.backward(list(outs), [T(z["grad_out." + n], torch.float32, DEV) for n in OUTS[name]])
    bwd = dwconv_func.launches["backward"] - before["backward"]
    refwd = dwconv_func.launches["forward"] - before["forward"] - fwd       # (a checkpointed block runs its forward again)
    return m, xs, outs, n_ffn, (fwd, refwd, bwd)


@pytest.mark.parametrize("on", [True, False])
@pytest.mark.parametrize("name", ["adapter_extractor", "adapter_interaction_cls"])
def test_blocks_fp32_against_the_reference_with_the_switch(name, on):
    """The bars test_vit_adapter_gpu.py holds: outputs 2e-5, input and parameter gradients 1e-4 of the largest reference
    entry; with the switch on the kernel runs once per ConvFFN forward and once per backward, off never."""
    z = load_fixture(name)
    m, xs, outs, n_ffn, counts = block_step(name, z, on)
    assert n_ffn >= 1 and counts == ((n_ffn, 0, n_ffn) if on else (0, 0, 0)), counts
    e_out = {n: rel(o, z["out." + n]) for n, o in zip(OUTS[name], outs)}
    e_in = {k: rel(x.grad, z["grad_in." + k]) for k, x in xs.items()}
    e_par = {k: rel(p.grad, z["grad." + k]) for k, p in m.named_parameters()}
    print(f"DWCONV-BLOCK {name} kernel={on} out {max(e_out.values()):.2e} grad_in {max(e_in.values()):.2e} "
          f"grad_param {max(e_par.values()):.2e}")
    assert all(v <= 2e-5 for v in e_out.values()), e_out
    assert all(v <= 1e-4 for v in e_in.values()), e_in
    assert all(v <= 1e-4 for v in e_par.values()), e_par


def test_with_cp_gives_bit_equal_outputs_with_the_switch_on():
    name = "adapter_interaction_cls"
    z = load_fixture(name)
    _, xs0, o0, n_ffn, c0 = block_step(name, z, True, with_cp=False)
    m1, xs1, o1, _, c1 = block_step(name, z, True, with_cp=True)
    assert c0 == (n_ffn, 0, n_ffn) and c1 == (n_ffn, n_ffn, n_ffn), (c0, c1)
    assert all(torch.equal(a, b) for a, b in zip(o0, o1))
    for k in xs0:                                          # (the bar of the existing checkpoint test)
        assert rel(xs1[k].grad, xs0[k].grad.double().cpu().numpy()) <= 1e-5, k


def test_extractor_forward_backward_replays_from_a_graph():
    """One forward + backward of an Extractor with the token kernel on, captured and replayed: bit-equal to the eager
    call (the level extents travel by value: nothing in the launch reads a table that capture could not see).
    Bit for bit holds for the output, the query's gradient and every parameter of the block but five tensors: grad_feat,
    feat_norm.{weight,bias} and attn.value_proj.{weight,bias} lie behind the op's fp32 grad_value, which at this geometry
    (336 queries on a 4 x 4 map) is not reproducible from one EAGER call to the next, whatever the convolution's route --
    measured with the switch off and on, four eager calls each: those five and only those differ, by 2.4e-7 .. 9.5e-6
    absolute (1e-6 .. 4e-6 of the largest entry), and the replays differ from an eager call by the same amounts.  They
    are held to the bar the existing checkpoint test sets for two runs of these blocks' gradients, 1e-5 of the largest
    entry; everything else, the whole ConvFFN with the kernel's three gradients included, to 0."""
    from mmfs_amd.blocks import DWConv, deform_inputs
    from mmfs_amd.functions import dwconv_func
    z = load_fixture("adapter_extractor")
    m = gpu_block("adapter_extractor", z, torch.float32).train()
    for mod in m.modules():
        if isinstance(mod, DWConv):
            mod.token_kernel = True
    h, w = (int(v) for v in z["image_hw"])
    _, d2 = deform_inputs(torch.zeros(1, 3, h, w, device=DEV))
    q = T(z["in.query"], torch.float32, DEV).requires_grad_(True)
    f = T(z["in.feat"], torch.float32, DEV).requires_grad_(True)
    grad = T(z["grad_out.out"], torch.float32, DEV)
    params = list(m.parameters())

    def step():
        out = m(q, d2[0], f, d2[1], d2[2], h // 16, w // 16)
        return (out,) + torch.autograd.grad(out, [q, f] + params, grad)

    before = dict(dwconv_func.launches)
    want = [t.detach().clone() for t in step()]
    assert dwconv_func.launches["forward"] == before["forward"] + 1 and dwconv_func.launches["backward"] == before["backward"] + 1
    assert rel(want[0], z["out.out"]) <= 2e-5
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    names = ["out", "grad_query", "grad_feat"] + [k for k, _ in m.named_parameters()]
    diffs = {n: float((a.detach().double() - b.double()).abs().max()) for n, a, b in zip(names, captured, want)}
    print("DWCONV-GRAPH-REPLAY max |replay - eager| " + (" ".join(f"{n} {v:.1e}" for n, v in diffs.items() if v > 0) or "all 0"))
    assert all(torch.isfinite(a).all() for a in captured)
    behind_grad_value = {"grad_feat", "feat_norm.weight", "feat_norm.bias", "attn.value_proj.weight", "attn.value_proj.bias"}
    assert {"ffn.dwconv.dwconv.weight", "ffn.dwconv.dwconv.bias", "ffn.fc1.weight", "ffn.fc2.weight"} <= set(names) - behind_grad_value
    assert all(v == 0.0 for n, v in diffs.items() if n not in behind_grad_value), {n: v for n, v in diffs.items() if v > 0}
    for n, a, b in zip(names, captured, want):
        if n in behind_grad_value:
            assert rel(a, b.double().cpu().numpy()) <= 1e-5, n


def test_conv_ffn_forward_backward_replays_from_a_graph_bit_for_bit():
    """ConvFFN alone (fc1 -> convolution + GELU -> fc2) in bf16 at three maps, forward + backward captured and replayed:
    every result equals the eager call's bit for bit, the kernel's weight and bias gradients included."""
    from mmfs_amd.blocks import ConvFFN
    from mmfs_amd.functions import dwconv_func
    torch.manual_seed(3)
    H = W = 8
    m = ConvFFN(64, 72).to(DEV, torch.bfloat16).train()
    m.dwconv.token_kernel = True
    x = torch.randn(3, 21 * (H // 2) * (W // 2), 64, device=DEV).to(torch.bfloat16).requires_grad_(True)
    grad = torch.randn_like(x)
    params = list(m.parameters())

    def step():
        out = m(x, H, W)
        return (out,) + torch.autograd.grad(out, [x] + params, grad)

    before = dict(dwconv_func.launches)
    want = [t.detach().clone() for t in step()]
    assert dwconv_func.launches == {"forward": before["forward"] + 1, "backward": before["backward"] + 1}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert all(torch.isfinite(a).all() for a in captured)
    assert all(torch.equal(a.detach(), b) for a, b in zip(captured, want))
