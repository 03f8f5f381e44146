"""The ViT-Adapter's output pyramid from the tokens (csrc/mmfs_pyramid.hip), host side: the C ABI's declarations, its
supported query and argument checks (every one returns before a launch, so they are safe without a GPU),
``AdapterPyramidHead`` on the CPU against the reference's fixture in fp64, and ``pyramid64`` -- this file's own fp64
restatement of the formulas, the yardstick of test_pyramid_head_gpu.py -- against the same fixture."""
import ctypes
import os
import re

import pytest
import torch

from test_vit_adapter import T, load_fixture, rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mmfs_msda.h")
NAMES = ("mmfs_pyramid_head_supported", "mmfs_pyramid_head_forward", "mmfs_pyramid_head_backward")
MASKS = [(0, 1, 2, 3), (1, 2, 3), (2,), (0, 3)]


from helpers import bound_library as _lib  # noqa: E402


# ------------------------------------------------------------------ the formulas, restated in fp64
def level_sizes(H, W):
    return [(4 * H, 4 * W), (2 * H, 2 * W), (H, W), (H // 2, W // 2)]


def resize_matrix(n, s):
    """[s n, n]: one axis of the bilinear resize by s (2 or 4), align_corners = False -- output o reads
    i0 = floor(src) and i1 = min(i0 + 1, n - 1) with 1 - f and f, src = max((o + 0.5) / s - 0.5, 0), f = src - i0."""
    M = torch.zeros(s * n, n, dtype=torch.float64)
    for o in range(s * n):
        src = max((o + 0.5) / s - 0.5, 0.0)
        i0 = int(src)
        f = src - i0
        M[o, i0] += 1.0 - f
        M[o, min(i0 + 1, n - 1)] += f
    return M


def mean_matrix(n):
    """[n / 2, n]: the resize by 0.5 is the mean of two"""
    M = torch.zeros(n // 2, n, dtype=torch.float64)
    for o in range(n // 2):
        M[o, 2 * o] = M[o, 2 * o + 1] = 0.5
    return M


def axis_matrices(H, W, device="cpu"):
    """per level the (rows, columns) matrices that take the H x W map to it (None: the identity)"""
    return [(resize_matrix(H, 4).to(device), resize_matrix(W, 4).to(device)),
            (resize_matrix(H, 2).to(device), resize_matrix(W, 2).to(device)), None,
            (mean_matrix(H).to(device), mean_matrix(W).to(device))]


def resample(x, H, W, mats):
    """x [B, HW, C] -> [B, h w, C]"""
    if mats is None:
        return x
    B, _, C = x.shape
    return torch.einsum("yi,xj,bijc->byxc", mats[0], mats[1], x.reshape(B, H, W, C)).reshape(B, -1, C)


def up64(c2, weight, bias):
    """adapter_up (ConvTranspose2d(C, C, 2, 2): weight [C, C, 2, 2]) as a GEMM on the tokens, columns (di, dj, o)"""
    C = weight.shape[0]
    return c2 @ weight.permute(0, 2, 3, 1).reshape(C, 4 * weight.shape[1]) + bias.repeat(4)


def up_pixels(up, H, W):
    """up [B, 4HW, 4C] -> the 4H x 4W map's tokens [B, 16HW, C]: pixel (2i + di, 2j + dj) <- row (i, j), block (di, dj)"""
    B, C = up.shape[0], up.shape[2] // 4
    return up.reshape(B, 2 * H, 2 * W, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, 16 * H * W, C)


def tokens_of(img):
    return img.flatten(2).transpose(1, 2)


def pyramid64(c, xs, up, c1, pos, H, W, levels=(0, 1, 2, 3)):
    """The four levels from the formulas, fp64, token-major: {l: [B, h_l w_l, C]}.  c [B, 21 HW / 4, C], xs four
    [B, HW, C], up [B, 4HW, 4C], c1 [B, C, 4H, 4W], pos four [h_l w_l, C] or None.  All weights are >= 0: on the absolute
    values of the inputs this is the sum of the absolute values of an element's terms."""
    mats = axis_matrices(H, W, c.device)
    n2, n3 = 4 * H * W, H * W
    base = {0: None, 1: c[:, :n2], 2: c[:, n2:n2 + n3], 3: c[:, n2 + n3:]}
    out = {}
    for l in levels:
        f = (up_pixels(up, H, W) + tokens_of(c1)) if l == 0 else base[l]
        f = f + resample(xs[l], H, W, mats[l])
        out[l] = f + pos[l] if pos is not None else f
    return out


def pyramid64_backward(g, H, W, c1_shape):
    """g {l: [B, h_l w_l, C]} -> the gradients of up, c1 (NCHW), x1..x4 ({l: ...}) by the issue's rules: permutation,
    transposition, the owner's gather with the forward's weights (the transposed matrices), copy, 0.25 x."""
    mats = axis_matrices(H, W, next(iter(g.values())).device)
    res = {"x": {}}
    for l, gl in g.items():
        B, _, C = gl.shape
        h, w = level_sizes(H, W)[l]
        if l == 0:
            res["up"] = gl.reshape(B, 2 * H, 2, 2 * W, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, 4 * H * W, 4 * C)
            res["c1"] = gl.transpose(1, 2).reshape(c1_shape)
        if mats[l] is None:
            res["x"][l] = gl
        else:
            res["x"][l] = torch.einsum("yi,xj,byxc->bijc", mats[l][0], mats[l][1], gl.reshape(B, h, w, C)).reshape(B, H * W, C)
    return res


def test_resize_matrices_are_the_frameworks_and_have_the_stated_phases():
    import torch.nn.functional as F
    for n in (2, 3, 6, 16):
        eye = torch.eye(n, dtype=torch.float64).reshape(n, 1, n, 1)       # n one-hot columns as images [n, 1, n, 1]
        for s in (2, 4):
            want = F.interpolate(eye, scale_factor=(s, 1), mode="bilinear", align_corners=False)[:, 0, :, 0].T
            assert torch.equal(resize_matrix(n, s), want), (n, s)
        if n % 2 == 0:
            want = F.interpolate(eye, scale_factor=(0.5, 1), mode="bilinear", align_corners=False)[:, 0, :, 0].T
            assert torch.equal(mean_matrix(n), want), n
    assert set(resize_matrix(6, 2)[2:-2].flatten().tolist()) == {0.0, 0.25, 0.75}
    assert set(resize_matrix(6, 4)[4:-4].flatten().tolist()) == {0.0, 0.125, 0.375, 0.625, 0.875}
    assert resize_matrix(6, 4)[0].tolist() == [1, 0, 0, 0, 0, 0] and resize_matrix(6, 4)[-1].tolist() == [0, 0, 0, 0, 0, 1]


# ------------------------------------------------------------------ the C ABI without a GPU
def test_new_symbols_are_declared_and_exported_at_abi_14():
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = _lib()
    for n in NAMES:
        assert re.search(r"\b" + n + r"\s*\(", text), n
        assert hasattr(lib, n), n
    assert lib.mmfs_msda_abi_version() == 14
    assert int(re.search(r"#define\s+MMFS_MSDA_ABI_VERSION\s+(\d+)", raw).group(1)) == 14


def test_supported_query():
    f = _lib().mmfs_pyramid_head_supported
    for dt, es in ((0, 4), (1, 2), (2, 2)):
        for C in (0, 4, 8, 12, 16, 36, 72, 256, 260, 1024):
            for H in (0, 1, 2, 3, 4, 6, 16):
                for W in (1, 2, 5, 10, 16):
                    for mask in (-1, 0, 1, 2, 7, 14, 15, 16):
                        want = int((C * es) % 16 == 0 and H >= 2 and W >= 2 and H % 2 == 0 and W % 2 == 0 and 1 <= mask <= 15)
                        assert f(dt, C, H, W, mask) == want, (dt, C, H, W, mask)
    assert f(3, 32, 4, 4, 15) == 0 and f(9, 32, 4, 4, 15) == 0 and f(-1, 32, 4, 4, 15) == 0        # fp64 / unknown dtype
    assert f(2, -8, 4, 4, 15) == 0 and f(2, 32, -4, 4, 15) == 0


def test_argument_errors_and_empty_problems_return_before_any_launch():
    lib = _lib()
    fake = ctypes.c_void_p(4096)                       # aligned, never dereferenced on these paths
    #       B  H  W   C  levels layout
    dims = [2, 4, 6, 32, 15, 0]

    def fwd(dt, dims, ptr=fake, **named):
        a = dict.fromkeys(("c", "x1", "x2", "x3", "x4", "up", "c1", "p1", "p2", "p3", "p4", "out"), ptr)
        a.update(named)
        return lib.mmfs_pyramid_head_forward(dt, *a.values(), *dims, None)

    def bwd(dt, dims, ptr=fake, **named):
        a = dict.fromkeys(("g", "up", "c1", "x1", "x2", "x3", "x4"), ptr)
        a.update(named)
        return lib.mmfs_pyramid_head_backward(dt, *a.values(), *dims, None)

    def with_(i, v):
        return dims[:i] + [v] + dims[i + 1:]

    for f in (fwd, bwd):
        assert f(9, dims) == -1 and f(3, dims) == -1 and f(-1, dims) == -1      # dtype (fp64 is not a storage type here)
        for i in (0, 1, 2, 3):
            assert f(2, with_(i, -2)) == -2                                     # negative B, H, W, C
        assert f(2, with_(1, 8192)) == -2 and f(2, with_(2, 8192)) == -2        # beyond the index range
        assert f(2, with_(1, 3)) == -5 and f(2, with_(2, 5)) == -5              # odd H, W
        assert f(2, with_(1, 0)) == -5 and f(2, with_(2, 0)) == -5              # H, W < 2
        assert f(2, with_(3, 12)) == -5 and f(0, with_(3, 6)) == -5             # C * sizeof(T) not a multiple of 16
        assert f(2, with_(4, 0)) == -5 and f(2, with_(4, 16)) == -5             # no level, an unknown level
        assert f(2, with_(5, 2)) == -5 and f(2, with_(5, -1)) == -5             # unknown c1 layout
        for i in (0, 3):                                                        # empty problems: nothing is looked at
            assert f(2, with_(i, 0), ptr=None) == 0
        assert f(2, dims, ptr=None) == -3                                       # NULL tensors of a non-empty problem
        assert f(2, dims, ptr=ctypes.c_void_p(4100)) == -4                      # tensors the 16-byte lanes cannot take
        for lay in (0, 1):
            assert f(2, with_(5, lay), ptr=ctypes.c_void_p(4100)) == -4
    # every required pointer by name; position tables may be absent; pointers of levels that are not selected too
    for name in ("c", "x1", "x2", "x3", "x4", "up", "c1", "out"):
        assert fwd(2, dims, **{name: None}) == -3, name
    assert bwd(2, dims, g=None) == -3
    # a NULL output of the backward is a gradient nobody needs; with all of them NULL nothing is left to launch
    assert bwd(2, dims, up=None, c1=None, x1=None, x2=None, x3=None, x4=None) == 0
    for name in ("up", "c1", "x1", "x2", "x3", "x4"):
        assert bwd(2, dims, ptr=ctypes.c_void_p(4100), **{name: None}) == -4, name
    assert fwd(2, with_(4, 14), up=None, c1=None, x1=None, p1=None, ptr=ctypes.c_void_p(4100)) == -4   # (reaches the last check)
    assert fwd(2, with_(4, 1), c=None, x2=None, x3=None, x4=None, ptr=ctypes.c_void_p(4100)) == -4
    assert bwd(2, with_(4, 4), up=None, c1=None, x1=None, x2=None, x4=None, ptr=ctypes.c_void_p(4100)) == -4
    assert fwd(2, with_(4, 14), x3=None) == -3
    # pointers of levels that are not selected are not looked at, alignment included
    odd = ctypes.c_void_p(4100)
    assert bwd(2, with_(4, 14), up=odd, c1=odd, x1=odd, x2=None, x3=None, x4=None) == 0
    assert bwd(2, with_(4, 14), up=odd, c1=odd, x1=odd, x2=odd, x3=None, x4=None) == -4
    assert fwd(2, dims, p1=None, p2=None, p3=None, p4=None, ptr=ctypes.c_void_p(4100)) == -4


# ------------------------------------------------------------------ the module on the CPU against the reference's fixture
def golden():
    z = load_fixture("adapter_pyramid")
    H = W = int(z["image_hw"][0]) // 16
    return z, H, W


def head_of(z, dtype=torch.float64, device="cpu"):
    from mmfs_amd.blocks import AdapterPyramidHead
    m = AdapterPyramidHead(int(z["in.c"].shape[2]))
    m.load_state_dict({k[len("param."):]: T(v) for k, v in z.items() if k.startswith("param.")}, strict=True)
    return m.to(device, dtype)


def inputs_of(z, dtype=torch.float64, device="cpu", grad=True):
    return {k[len("in."):]: T(v, dtype, device).requires_grad_(grad) for k, v in z.items() if k.startswith("in.")}


def packed_grad(z, levels, dtype=torch.float64, device="cpu"):
    return torch.cat([tokens_of(T(z[f"grad_out.l{l}"], dtype, device)) for l in levels], 1)


@pytest.mark.parametrize("with_pos", [False, True])
@pytest.mark.parametrize("packed", [True, False])
@pytest.mark.parametrize("levels", MASKS)
def test_head_matches_the_reference_in_fp64(levels, packed, with_pos):
    """Outputs of every mask, and for the full mask all input and ``adapter_up`` gradients, within 1e-12 of each array's
    largest entry (measured worst over the cases: 1.1e-15).  The gradients of a partial mask are held
    against ``pyramid64`` under autograd (the fixture's are those of all four levels), which
    test_pyramid64_matches_the_reference ties to the fixture."""
    worst = [0.0]

    def held(e, what):
        worst[0] = max(worst[0], e)
        assert e <= 1e-12, (what, e)

    z, H, W = golden()
    m = head_of(z)
    x = inputs_of(z)
    xs = [x[f"x{k}"] for k in range(1, 5)]
    pos = T(z["pos_embed"], None) if with_pos else None
    out = m(x["c"], xs, x["c1"], H, W, pos_embed=pos, levels=levels, packed=packed)
    key = "out_pos.l" if with_pos else "out.l"
    if packed:
        assert tuple(out.shape) == (2, sum(h * w for l, (h, w) in enumerate(level_sizes(H, W)) if l in levels), x["c"].shape[2])
        want = torch.cat([tokens_of(T(z[key + str(l)])) for l in levels], 1)
        held(rel(out, want.numpy()), "packed")
        out.backward(packed_grad(z, levels))
    else:
        assert len(out) == len(levels)
        for l, f in zip(levels, out):
            assert tuple(f.shape) == tuple(z[key + str(l)].shape)
            held(rel(f, z[key + str(l)]), l)
        torch.autograd.backward(list(out), [T(z[f"grad_out.l{l}"]) for l in levels])
    grads = {"c": x["c"].grad, "c1": x["c1"].grad, **{f"x{k}": x[f"x{k}"].grad for k in range(1, 5)}}
    pgrads = {k: p.grad for k, p in m.named_parameters()}
    if levels == (0, 1, 2, 3):
        for k, g in grads.items():
            held(rel(g, z["grad_in." + k]), k)
        for k, g in pgrads.items():
            held(rel(g, z["grad." + k]), k)
        print(f"PYRAMID-HEAD-FP64 levels={levels} packed={packed} pos={with_pos} worst {worst[0]:.2e}")
        return
    y = inputs_of(z)
    w, b = (T(z["param.adapter_up." + k]).requires_grad_(True) for k in ("weight", "bias"))
    tabs = [T(z[f"pos.l{l}"]) for l in range(4)] if with_pos else None
    ref = pyramid64(y["c"], [y[f"x{k}"] for k in range(1, 5)], up64(y["c"][:, :4 * H * W], w, b), y["c1"], tabs, H, W, levels)
    torch.cat([ref[l] for l in levels], 1).backward(packed_grad(z, levels))
    for k, g in grads.items():
        if y[k].grad is None:
            assert g is None or not g.any(), k          # an input of levels that are not produced gets no gradient
        else:
            held(rel(g, y[k].grad.numpy()), k)
    for k, g, r in (("weight", pgrads["adapter_up.weight"], w.grad), ("bias", pgrads["adapter_up.bias"], b.grad)):
        assert (g is None) == (r is None), k
        if g is not None:
            held(rel(g, r.numpy()), k)
    print(f"PYRAMID-HEAD-FP64 levels={levels} packed={packed} pos={with_pos} worst {worst[0]:.2e}")


def test_pyramid64_matches_the_reference():
    """This file's restatement of the formulas -- the GPU tests' yardstick -- against the fixture: outputs without and
    with the tables, and the backward rules (g_up through the GEMM gives the parameter and c2 gradients), all within
    1e-12 of each array's largest entry (measured worst: 1.1e-15)."""
    z, H, W = golden()
    x = inputs_of(z, grad=False)
    xs = [x[f"x{k}"] for k in range(1, 5)]
    w, b = (T(z["param.adapter_up." + k]).requires_grad_(True) for k in ("weight", "bias"))
    c2 = x["c"][:, :4 * H * W].clone().requires_grad_(True)
    up = up64(c2, w, b)
    tabs = [T(z[f"pos.l{l}"]) for l in range(4)]
    worst = 0.0
    for key, pos in (("out.l", None), ("out_pos.l", tabs)):
        got = pyramid64(x["c"], xs, up.detach(), x["c1"], pos, H, W)
        for l in range(4):
            e = rel(got[l], tokens_of(T(z[key + str(l)])).numpy())
            worst = max(worst, e)
            assert e <= 1e-12, (key, l)
    g = {l: tokens_of(T(z[f"grad_out.l{l}"])) for l in range(4)}
    back = pyramid64_backward(g, H, W, x["c1"].shape)
    up.backward(back["up"])
    g_c = torch.cat([g[1] + c2.grad, g[2], g[3]], 1)         # levels 2..4 of g itself, + the GEMM's share of c2
    checks = [(g_c, "grad_in.c"), (back["c1"], "grad_in.c1"), (w.grad, "grad.adapter_up.weight"), (b.grad, "grad.adapter_up.bias")]
    checks += [(back["x"][l], f"grad_in.x{l + 1}") for l in range(4)]
    for got, name in checks:
        e = rel(got, z[name])
        worst = max(worst, e)
        assert e <= 1e-12, name
    print(f"PYRAMID64 worst relative difference to the fixture {worst:.2e}")


def test_position_tables_are_the_references_and_kept():
    from mmfs_amd.blocks import pyramid_pos_tables
    z, H, W = golden()
    pe = T(z["pos_embed"], None)
    tabs = pyramid_pos_tables(pe, H, W)
    assert pyramid_pos_tables(pe, H, W) is tabs and pyramid_pos_tables(pe[1:].contiguous(), H, W) is not tabs
    for l, t in enumerate(tabs):
        assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == tuple(z[f"pos.l{l}"].shape)
        # (the framework's bicubic kernel in fp32: a CPU's vector width may place its roundings differently from the
        # machine the fixture was made on -- a few ulp of entries of at most ~1.3)
        assert float((t - T(z[f"pos.l{l}"], None)).abs().max()) <= 2e-6, l
    for a, b in zip(pyramid_pos_tables(pe[1:].contiguous(), H, W), tabs):
        assert torch.equal(a, b)
    with pytest.raises(ValueError):
        pyramid_pos_tables(pe, 4, 6)


def test_state_dict_keys_are_the_references():
    from mmfs_amd.blocks import AdapterPyramidHead
    for on in (True, False):
        m = AdapterPyramidHead(16)
        m.token_kernel = on
        sd = m.state_dict()
        assert set(sd) == {"adapter_up.weight", "adapter_up.bias"}
        assert tuple(sd["adapter_up.weight"].shape) == (16, 16, 2, 2) and tuple(sd["adapter_up.bias"].shape) == (16,)
    # mounted where the reference has it, ``vision_model.adapter_up.*`` loads unchanged
    class Vision(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.vision_model = AdapterPyramidHead(16)
    ref = {"vision_model.adapter_up.weight": torch.randn(16, 16, 2, 2), "vision_model.adapter_up.bias": torch.randn(16)}
    Vision().load_state_dict(ref, strict=True)


def test_packed_result_feeds_the_bank_like_the_level_list_bit_for_bit():
    from mmfs_amd import bank
    z, H, W = golden()
    x = inputs_of(z, torch.float32, grad=False)
    xs = [x[f"x{k}"] for k in range(1, 5)]
    m = head_of(z, torch.float32)
    pe = T(z["pos_embed"], None)
    # 4 images as two copies of the fixture's two
    c, c1 = torch.cat((x["c"], x["c"].flip(0))), torch.cat((x["c1"], x["c1"].flip(0)))
    xs = [torch.cat((t, t.flip(0))) for t in xs]
    num = torch.tensor([1, 3])
    text = torch.tensor([[1, 5, 7, 9, 9, 9, 9, 9], [1, 5, 7, 5, 7, 5, 7, 9]])
    with torch.no_grad():
        feats = m(c, xs, c1, H, W, pos_embed=pe, packed=False)
        want = bank.prepare_mmfs_features_for_mm_decoder(text, num, feats, bos_token_id=1, soi_token_id=5,
                                                         spatial_shapes=[2 * H, H, H // 2], max_num_image=3)["mmfs_features_mm"]
        packed = m(c, xs, c1, H, W, pos_embed=pe, levels=(1, 2, 3))
        got = bank.llm_feature_bank(packed, num, 3)
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, 3, 21 * H * W // 4, c.shape[2])
    assert torch.equal(got, want)
    assert torch.equal(packed, bank.pack_image_levels(feats, [2 * H, H, H // 2]))


def test_cpu_tensors_take_the_framework_path_whatever_the_switch_says(monkeypatch):
    import mmfs_amd.blocks.vit_adapter as va
    assert isinstance(va.AdapterPyramidHead.token_kernel, bool)

    def boom(*a):
        raise AssertionError("the token kernel was called on CPU tensors")

    monkeypatch.setattr(va.PyramidHeadFunction, "apply", boom)
    z, H, W = golden()
    x = inputs_of(z, torch.float32, grad=False)
    xs = [x[f"x{k}"] for k in range(1, 5)]
    res = {}
    for on in (True, False):
        m = head_of(z, torch.float32)
        m.token_kernel = on
        res[on] = m(x["c"], xs, x["c1"], H, W)
    assert torch.equal(res[True], res[False])
    with pytest.raises(ValueError):
        head_of(z)(x["c"], xs, x["c1"], H, W, levels=())


def test_function_is_exported():
    from mmfs_amd import blocks, functions
    assert hasattr(functions, "PyramidHeadFunction") and hasattr(functions, "pyramid_head_supported")
    assert hasattr(blocks, "AdapterPyramidHead") and hasattr(blocks, "pyramid_pos_tables")
    c = torch.zeros(1, 21, 8)
    xs = [torch.zeros(1, 4, 8)] * 4
    assert functions.pyramid_head_supported(c, xs, torch.zeros(1, 8, 8, 8), None, 2, 2, 15) is False      # CPU tensors
