"""ConvFFN's depthwise convolution in the token layout (csrc/msda_dwconv.hip), host side: the C ABI's declarations,
its supported query and argument checks (every one returns before a launch, so they are safe without a GPU), and the
blocks' switch -- on the CPU ``DWConv`` / ``ConvFFN`` run the reference's framework statement whatever the switch
says, and the state dict never changes.  The kernels themselves are held in test_dwconv_gpu.py."""
import ctypes
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mmfs_msda.h")
NAMES = ("mmfs_dwconv_tokens_supported", "mmfs_dwconv_tokens_forward", "mmfs_dwconv_tokens_backward_workspace_bytes",
         "mmfs_dwconv_tokens_backward")


from helpers import bound_library as _lib  # noqa: E402


def test_new_symbols_are_declared_and_exported_at_abi_14():
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = _lib()
    for n in NAMES:
        assert re.search(r"\b" + n + r"\s*\(", text), n
        assert hasattr(lib, n), n
    assert lib.mmfs_msda_abi_version() == 14
    assert int(re.search(r"#define\s+MMFS_MSDA_ABI_VERSION\s+(\d+)", raw).group(1)) == 14
    assert "mmfs_dwconv_tokens_supported" in raw[raw.index("#define MMFS_MSDA_ABI_VERSION"):raw.index("enum mmfs_dtype")]


def test_supported_query():
    f = _lib().mmfs_dwconv_tokens_supported
    for dt, es in ((0, 4), (1, 2), (2, 2)):
        for C in (0, 4, 8, 12, 16, 32, 36, 72, 256, 260):
            for L in (0, 1, 3, 8, 9):
                for act in (-1, 0, 1, 2):
                    want = int((C * es) % 16 == 0 and 1 <= L <= 8 and act in (0, 1))
                    assert f(dt, C, L, act) == want, (dt, C, L, act)
    assert f(3, 32, 3, 0) == 0 and f(9, 32, 3, 0) == 0 and f(-1, 32, 3, 0) == 0        # fp64 / unknown dtype
    assert f(2, -8, 3, 0) == 0


def test_argument_errors_and_empty_problems_return_before_any_launch():
    lib = _lib()
    fake = ctypes.c_void_p(4096)                       # aligned, never dereferenced on these paths
    hw = (ctypes.c_int64 * 6)(8, 8, 4, 4, 2, 2)        # 84 tokens
    #       B   N   C  L  act
    dims = [2, 84, 32, 3, 1]

    def fwd(dt, dims, ptr=fake, level_hw=hw):
        B, N, C, L, act = dims
        return lib.mmfs_dwconv_tokens_forward(dt, ptr, ptr, ptr, ptr, ptr, level_hw, B, N, C, L, act, None)

    def bwd(dt, dims, ptr=fake, level_hw=hw):
        B, N, C, L, act = dims
        return lib.mmfs_dwconv_tokens_backward(dt, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, level_hw, B, N, C, L, act, None)

    def wsb(dt, dims, ptr=fake, level_hw=hw):
        B, N, C, L, act = dims
        return lib.mmfs_dwconv_tokens_backward_workspace_bytes(dt, level_hw, B, N, C, L, act)

    def with_(i, v):
        return dims[:i] + [v] + dims[i + 1:]

    for f in (fwd, bwd, wsb):
        assert f(9, dims) == -1 and f(3, dims) == -1 and f(-1, dims) == -1      # dtype (fp64 is not a storage type here)
        for i in (0, 1, 2):
            assert f(2, with_(i, -1)) == -2                                     # negative B, N, C
        assert f(2, dims, level_hw=(ctypes.c_int64 * 6)(8, 8, 4, 4, 0, 4)) == -2         # a non-positive extent
        assert f(2, dims, level_hw=(ctypes.c_int64 * 6)(8, 8, 4, 4, -2, -2)) == -2
        assert f(2, dims, level_hw=(ctypes.c_int64 * 6)(8, 8, 4, 4, 2, 3)) == -2         # sum h * w != N
        assert f(2, with_(1, 85)) == -2
        assert f(2, with_(3, 0)) == -5 and f(2, with_(3, 9)) == -5              # L outside [1, 8]
        assert f(2, with_(2, 12)) == -5 and f(0, with_(2, 6)) == -5             # C * sizeof(T) not a multiple of 16
        assert f(2, with_(4, 2)) == -5 and f(2, with_(4, -1)) == -5             # unknown act
        assert f(2, dims, level_hw=None) == -3                                  # the host table of a non-empty problem
        for i in (0, 1, 2):                                                     # empty problems: nothing is looked at
            assert f(2, with_(i, 0), ptr=None, level_hw=None) == 0
    for f in (fwd, bwd):
        assert f(2, dims, ptr=None) == -3                                       # NULL tensors of a non-empty problem
        assert f(2, dims, ptr=ctypes.c_void_p(4100)) == -4                      # tensors the 16-byte lanes cannot take
    # the workspace of the two-stage weight-gradient reduction: one fp32 row [10, C] per workgroup of the first stage
    # (csrc/msda_dwconv.hip: 4-channel lanes, strips of 16 rows)
    assert wsb(2, dims) == _ws_rows(2, [(8, 8), (4, 4), (2, 2)], 32) * 10 * 32 * 4
    assert wsb(0, [3, 1344, 256, 3, 0], level_hw=(ctypes.c_int64 * 6)(32, 32, 16, 16, 8, 8)) == \
        _ws_rows(3, [(32, 32), (16, 16), (8, 8)], 256) * 10 * 256 * 4


def _ws_rows(B, maps, C):
    clb = 1
    while clb < min(C // 4, 256):
        clb *= 2
    items = B * sum(-(-h // 16) * w for h, w in maps)
    return -(-items // (256 // clb))


def _blocks():
    from mmfs_amd.blocks import ConvFFN, DWConv
    return ConvFFN, DWConv


def test_cpu_tensors_take_the_framework_path_whatever_the_switch_says(monkeypatch):
    ConvFFN, DWConv = _blocks()
    import mmfs_amd.blocks.vit_adapter as va
    assert isinstance(DWConv.token_kernel, bool)

    def boom(*a):
        raise AssertionError("the token kernel was called on CPU tensors")

    monkeypatch.setattr(va.DWConvTokensFunction, "apply", boom)
    torch.manual_seed(0)
    H = W = 4
    N = 21 * (H // 2) * (W // 2)
    x = torch.randn(2, N, 24, dtype=torch.float64)
    conv, ffn = DWConv(16).double(), ConvFFN(24, 16).double()
    res = {}
    for on in (True, False):
        monkeypatch.setattr(DWConv, "token_kernel", on)
        assert conv.tokens(x[..., :16], H, W, "none") is None
        a = conv(x[..., :16].contiguous(), H, W)
        b = ffn(x, H, W)
        res[on] = (a, b)
    assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1])
    # ... and it is the reference's statement: each map convolved as an image
    xs = x[..., :16].contiguous()
    parts, lo = [], 0
    for hh, ww in ((2 * H, 2 * W), (H, W), (H // 2, W // 2)):
        img = xs[:, lo:lo + hh * ww].transpose(1, 2).reshape(2, 16, hh, ww)
        parts.append(torch.nn.functional.conv2d(img, conv.dwconv.weight, conv.dwconv.bias, 1, 1, 1, 16).flatten(2).transpose(1, 2))
        lo += hh * ww
    assert torch.equal(res[True][0], torch.cat(parts, 1))


def test_the_switch_leaves_the_state_dict_alone(monkeypatch):
    ConvFFN, DWConv = _blocks()
    keys = {"fc1.weight", "fc1.bias", "dwconv.dwconv.weight", "dwconv.dwconv.bias", "fc2.weight", "fc2.bias"}
    for on in (True, False):
        monkeypatch.setattr(DWConv, "token_kernel", on)
        m = ConvFFN(32, 8)
        sd = m.state_dict()
        assert set(sd) == keys
        assert tuple(sd["dwconv.dwconv.weight"].shape) == (8, 1, 3, 3) and tuple(sd["dwconv.dwconv.bias"].shape) == (8,)
        ConvFFN(32, 8).load_state_dict(sd, strict=True)
    m = DWConv(8)
    m.token_kernel = False
    assert set(m.state_dict()) == {"dwconv.weight", "dwconv.bias"}


def test_function_is_exported():
    from mmfs_amd import functions
    assert hasattr(functions, "DWConvTokensFunction") and hasattr(functions, "dwconv_tokens_supported")
    x = torch.zeros(1, 21, 8)
    conv = torch.nn.Conv2d(8, 8, 3, 1, 1, groups=8)
    assert functions.dwconv_tokens_supported(x, conv.weight, conv.bias) is False        # CPU tensors
