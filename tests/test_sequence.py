"""The interleaved sequence (mmfs_amd/sequence.py, csrc/mmfs_sequence.hip), host side: the framework route in fp64 against
the reference's fixtures (tests/golden/sequence_*.npz, made by tests/golden/make_golden_sequence.py from the reference's
two methods), values and gradients; the sin-cos table bit for bit; the tables against a plain loop; the C ABI's
declarations and its argument checks (every one returns before a launch, so they are safe without a GPU)."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from helpers import load_golden

import mmfs_amd
from mmfs_amd import sequence as seq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mmfs_msda.h")
NAMES = ("mmfs_sequence_supported", "mmfs_sequence_index", "mmfs_sequence_embed_forward", "mmfs_sequence_embed_backward",
         "mmfs_sequence_context_forward", "mmfs_sequence_context_backward", "mmfs_sequence_context_backward_workspace_bytes")
CASES = ("sequence_bos", "sequence_start")
BAR = 1e-12


def fixture(name):
    g = {k: torch.from_numpy(np.asarray(v)) for k, v in load_golden(name).items()}
    for k, v in g.items():
        if v.dtype == torch.float32 and k != "pos_table":
            g[k] = v.double()                                   # (stored as fp32 where that is lossless)
    g["bos_id"], g["soi_id"], g["image_id"] = (int(x) for x in g["special_ids"])
    return g


def projection(g, dtype=torch.float64, device="cpu"):
    w = g["weight"].to(device=device, dtype=dtype).requires_grad_(True)
    b = g["bias"].to(device=device, dtype=dtype).requires_grad_(True)
    return types.SimpleNamespace(weight=w, bias=b)


def context_call(g, x, proj, **kw):
    n = kw.setdefault("n_images", 4)

    def per_image(t):                                           # (a slot beyond the fixture's four images: any entry)
        return None if t is None else torch.cat((t, t.new_zeros(max(n - 4, 0))))[:n].to(x.device)
    return seq.prepare_context_features_for_image_decoder(
        x, g["text_ids"].to(x.device), proj, soi_token_id=g["soi_id"], seq_len=int(g["seq_len"]),
        nearest_bos_idxs=per_image(g.get("nearest_bos_idxs")),
        image_start_token_idx=per_image(g.get("image_start_token_idx")), **kw)


def err(a, b):
    return float((a.detach().double() - b.detach().double()).abs().max())


# ------------------------------------------------------------------ the tables
def loop_tables(ids, image_id, soi_id, n_vis, n_images):
    """the tables of csrc/mmfs_sequence.hip's header, token by token"""
    B, L = ids.shape
    rank, pos = [-1] * (B * L), [-1] * n_vis
    row, col, first = [-1] * n_images, [-1] * n_images, [0] * (B + 1)
    n_img = n_soi = 0
    for t, v in enumerate(ids.reshape(-1).tolist()):
        if L and t % L == 0:
            first[t // L] = min(n_soi, n_images)
        if v == image_id:
            if n_img < n_vis:
                rank[t], pos[n_img] = n_img, t
            n_img += 1
        if v == soi_id:
            if n_soi < n_images:
                row[n_soi], col[n_soi] = t // L, t % L
            n_soi += 1
    first[B] = min(n_soi, n_images)
    return rank, pos, row, col, first, [n_img, n_soi]


def index_layouts():
    """(name, ids, image id, soi id): the layouts the index must get right -- a single token, 2049 tokens (across a scan
    chunk), no image token, image tokens at the first and last flat position, <soi> at column 0 and L - 1"""
    gen = torch.Generator().manual_seed(5)
    out = []
    one = torch.full((1, 1), 7)
    out.append(("single_image_token", one, 7, 9))
    out.append(("single_soi", one, 3, 7))
    ids = torch.randint(0, 6, (3, 683), generator=gen)           # ids 4 = image, 5 = <soi>: dense
    ids[0, 0] = 4
    ids[2, 682] = 4
    ids[1, 0] = 5
    ids[1, 682] = 5
    out.append(("dense_2049", ids, 4, 5))
    out.append(("no_image_token", ids, 77, 5))
    out.append(("no_soi", ids, 4, 77))
    sparse = torch.randint(10, 50, (2, 40), generator=gen)
    sparse[0, 0], sparse[0, 39], sparse[1, 0], sparse[1, 39] = 5, 4, 4, 5
    sparse[1, 20:24] = 4
    out.append(("sparse_edges", sparse, 4, 5))
    return out


def assert_tables(t, ids, image_id, soi_id, n_vis, n_images):
    want = loop_tables(ids, image_id, soi_id, n_vis, n_images)
    for name, got, ref in zip(("img_rank", "img_pos", "soi_row", "soi_col", "row_first", "counts"), t[:6], want):
        assert got.dtype == torch.int32, name
        assert got.cpu().tolist() == ref, name


@pytest.mark.parametrize("layout", index_layouts(), ids=lambda l: l[0])
def test_tables_match_a_plain_loop(layout):
    _, ids, image_id, soi_id = layout
    n_img, n_soi = int((ids == image_id).sum()), int((ids == soi_id).sum())
    for n_vis, n_images in ((n_img, n_soi), (n_img + 1, n_soi + 1), (max(n_img - 1, 0), max(n_soi - 1, 0))):
        t = seq.sequence_tables(ids, image_token_id=image_id, soi_token_id=soi_id, n_vis=n_vis, n_images=n_images)
        assert_tables(t, ids, image_id, soi_id, n_vis, n_images)


# ------------------------------------------------------------------ against the reference's fixtures, fp64
def test_sincos_table_is_the_references_bit_for_bit():
    g = fixture(CASES[0])
    t = seq.sincos_1d_table(int(g["seq_len"]), g["pos_table"].shape[1], torch.float32, "cpu")
    assert t.dtype == torch.float32 and torch.equal(t, g["pos_table"])
    assert np.array_equal(t.numpy().view(np.uint32), g["pos_table"].numpy().view(np.uint32))


def test_invalidate_caches_drops_the_table():
    a = seq.sincos_1d_table(32, 16, torch.float32, "cpu")
    assert seq.sincos_1d_table(32, 16, torch.float32, "cpu") is a
    mmfs_amd.invalidate_caches()
    b = seq.sincos_1d_table(32, 16, torch.float32, "cpu")
    assert b is not a and torch.equal(a, b)


def embed_call(g, text, vis, soi, **kw):
    return seq.assemble_mm_embeds(text, g["text_ids"].to(text.device), vis, soi, image_token_id=g["image_id"],
                                  soi_token_id=g["soi_id"], **kw)


def test_mm_embeds_and_gradients_against_the_fixture():
    g = fixture(CASES[0])
    text, vis, soi = (g[k].clone().requires_grad_(True) for k in ("text_embeds", "vis_embed", "soi_token"))
    out = embed_call(g, text, vis, soi, validate=True)
    assert out.dtype == torch.float64 and out.shape == g["mm_embeds"].shape
    assert err(out, g["mm_embeds"]) <= BAR
    out.backward(g["grad_out.mm_embeds"])
    for name, leaf in (("text_embeds", text), ("vis_embed", vis), ("soi_token", soi)):
        assert leaf.grad.shape == g["grad." + name].shape
        assert err(leaf.grad, g["grad." + name]) <= BAR, name


def test_mm_embeds_validation_and_surplus_rows():
    g = fixture(CASES[0])
    text, soi = g["text_embeds"], g["soi_token"]
    more = torch.cat((g["vis_embed"].reshape(-1, 16), torch.ones(2, 16, dtype=torch.float64))).requires_grad_(True)
    with pytest.raises(AssertionError):
        embed_call(g, text, more, soi, validate=True)
    out = embed_call(g, text, more, soi)
    assert err(out, g["mm_embeds"]) <= BAR
    out.backward(g["grad_out.mm_embeds"])
    assert err(more.grad[:6], g["grad.vis_embed"].reshape(-1, 16)) <= BAR and float(more.grad[6:].abs().max()) == 0.0
    fewer = g["vis_embed"].reshape(-1, 16)[:4]                   # the last two image tokens keep their text embedding
    out = embed_call(g, text, fewer, soi)
    ids = g["text_ids"]
    keep = torch.ones_like(ids, dtype=torch.bool)
    keep[2, 2:4] = False
    assert err(out[keep], g["mm_embeds"][keep]) <= BAR and err(out[2, 2:4], text[2, 2:4]) <= BAR


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("order", ["project_first", "gather_first", "auto"])
def test_context_features_and_gradients_against_the_fixture(case, order):
    g = fixture(case)
    x = g["context_features"].clone().requires_grad_(True)
    proj = projection(g)
    feats, mask = context_call(g, x, proj, order=order)
    assert mask.dtype == torch.long and torch.equal(mask, g["mask"])
    assert feats.dtype == torch.float64 and feats.shape == g["features"].shape
    assert err(feats, g["features"]) <= BAR
    feats.backward(g["grad_out.features"])
    for name, leaf in (("context_features", x), ("weight", proj.weight), ("bias", proj.bias)):
        assert err(leaf.grad, g["grad." + name]) <= BAR, name


@pytest.mark.parametrize("case", CASES)
def test_the_two_orders_agree_and_max_len_cuts_and_pads(case):
    g = fixture(case)
    x, proj = g["context_features"], projection(g)
    with torch.no_grad():
        a, ma = context_call(g, x, proj, order="project_first", max_len=24)
        b, mb = context_call(g, x, proj, order="gather_first", max_len=24)
        assert err(a, b) <= BAR and torch.equal(ma, mb) and err(a, g["features"]) <= BAR
        for order in ("project_first", "gather_first"):
            cut, mc = context_call(g, x, proj, order=order, max_len=5)                  # below the longest context
            assert err(cut, g["features"][:, :5]) <= BAR and torch.equal(mc, g["mask"][:, :5])
            pad, mp = context_call(g, x, proj, order=order, max_len=30, n_images=5)     # above it, and one slot too many
            pos = g["pos_table"].double()
            assert err(pad[:4, :24], g["features"]) <= BAR and torch.equal(mp[:4, :24], g["mask"])
            assert err(pad[:, 24:], (proj.bias + pos[24:30]).expand(5, 6, 16)) <= BAR and int(mp[:, 24:].sum()) == 0
            assert err(pad[4], proj.bias + pos[:30]) <= BAR and int(mp[4].sum()) == 0
        with pytest.raises(ValueError):
            context_call(g, x, proj, max_len=33)                                        # beyond seq_len
        with pytest.raises(ValueError):                                                 # one entry per slot, not per <soi>
            seq.prepare_context_features_for_image_decoder(x, g["text_ids"], proj, soi_token_id=g["soi_id"], seq_len=32,
                                                           n_images=5, nearest_bos_idxs=torch.zeros(4, dtype=torch.long))


def test_a_padded_row_does_not_see_the_weight():
    """the one deviation: project_first's padding is bias + pos, whatever the weight holds"""
    g = fixture(CASES[0])
    proj = projection(g)
    with torch.no_grad():
        proj.weight[3, 5] = float("inf")
        feats, mask = context_call(g, g["context_features"], proj, order="project_first")
    pad = ~mask.bool()
    want = (proj.bias + g["pos_table"].double()[:24]).expand(4, 24, 16)
    assert torch.isfinite(feats[pad]).all() and err(feats[pad], want[pad]) <= BAR


def test_a_forced_kernel_route_on_host_tensors_is_an_error():
    g = fixture(CASES[0])
    with pytest.raises(RuntimeError):
        context_call(g, g["context_features"], projection(g), route="kernels")
    with pytest.raises(RuntimeError):
        embed_call(g, g["text_embeds"], g["vis_embed"], g["soi_token"], route="kernels")


# ------------------------------------------------------------------ the C ABI without a GPU
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
    assert "mmfs_sequence_supported" in raw[raw.index("#define MMFS_MSDA_ABI_VERSION"):raw.index("enum mmfs_dtype")]


def test_supported_query_refuses_odd_widths():
    f = _lib().mmfs_sequence_supported
    for dt, es in ((0, 4), (1, 2), (2, 2)):
        for C in (-8, 0, 1, 2, 4, 6, 8, 12, 16, 20, 24, 136, 4096, 4100):
            assert f(dt, C) == int(C > 0 and (C * es) % 16 == 0), (dt, C)
    assert f(3, 32) == 0 and f(9, 32) == 0 and f(-1, 32) == 0           # fp64 / unknown dtype


def test_argument_errors_return_before_any_launch():
    lib = _lib()
    fake, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)            # never dereferenced on these paths
    DTYPE, DIMS, NULLPTR, ALIGN, UNSUPPORTED = -1, -2, -3, -4, -5

    def index(B=2, L=8, n_vis=3, n_images=2, **named):
        p = dict.fromkeys(("rank", "pos", "row", "col", "first", "counts"), fake)
        p.update({k: v for k, v in named.items() if k in p})
        return lib.mmfs_sequence_index(named.get("ids", fake), B, L, 4, 5, n_vis, n_images, *p.values(), None)

    assert index(B=-1) == DIMS and index(L=-1) == DIMS and index(n_vis=-1) == DIMS and index(n_images=-1) == DIMS
    assert index(B=4, L=(1 << 20) + 1) == DIMS and index(n_vis=(1 << 22) + 1) == DIMS
    assert index(ids=None) == NULLPTR and index(first=None) == NULLPTR and index(counts=None) == NULLPTR
    assert index(row=None) == NULLPTR and index(pos=None) == NULLPTR
    assert index(ids=odd) == ALIGN and index(rank=ctypes.c_void_p(4098)) == ALIGN

    def embed_fwd(dt=2, tdt=2, rows=16, C=32, n_vis=3, **named):
        p = dict.fromkeys(("text", "vis", "soi", "ids", "rank", "out"), fake)
        p.update(named)
        return lib.mmfs_sequence_embed_forward(dt, tdt, p["text"], p["vis"], p["soi"], p["ids"], 5, p["rank"], p["out"],
                                               rows, C, n_vis, None)

    def embed_bwd(dt=2, tdt=2, rows=16, C=32, n_vis=3, L=8, n_images=2, **named):
        p = dict.fromkeys(("grad", "rank", "pos", "row", "col", "counts", "g_text", "g_vis", "g_soi"), fake)
        p.update(named)
        return lib.mmfs_sequence_embed_backward(dt, tdt, *p.values(), rows, L, C, n_vis, n_images, None)

    for f in (embed_fwd, embed_bwd):
        assert f(dt=9) == DTYPE and f(dt=3) == DTYPE and f(tdt=7) == DTYPE
        assert f(rows=-1) == DIMS and f(C=-8) == DIMS and f(n_vis=-1) == DIMS and f(rows=(1 << 22) + 8) == DIMS
        assert f(C=12) == UNSUPPORTED and f(dt=0, tdt=0, C=6) == UNSUPPORTED and f(C=0) == UNSUPPORTED
        assert f(dt=2, tdt=1) == UNSUPPORTED                                # text is neither T nor fp32
    assert embed_fwd(text=None) == NULLPTR and embed_fwd(out=None) == NULLPTR and embed_fwd(rank=None) == NULLPTR
    assert embed_fwd(vis=odd) == ALIGN and embed_fwd(rows=0, text=None) == 0
    assert embed_bwd(grad=None) == NULLPTR and embed_bwd(counts=None) == NULLPTR and embed_bwd(g_soi=odd) == ALIGN
    assert embed_bwd(rows=15) == DIMS and embed_bwd(L=-1) == DIMS
    assert embed_bwd(g_text=None, g_vis=None, g_soi=None, grad=None) == 0     # no gradient is wanted

    def ctx_fwd(dt=2, B=2, L=8, C=32, n_images=3, max_len=4, seq_len=16, **named):
        p = dict.fromkeys(("src", "pad", "pos", "row", "col", "start", "bos", "out", "mask"), fake)
        p.update(named)
        return lib.mmfs_sequence_context_forward(dt, *p.values(), B, L, C, n_images, max_len, seq_len, None)

    def ctx_bwd(dt=2, B=2, L=8, C=32, n_images=3, max_len=4, seq_len=16, **named):
        p = dict.fromkeys(("grad", "row", "col", "first", "start", "bos", "g_src", "g_pad", "ws"), fake)
        p.update(named)
        return lib.mmfs_sequence_context_backward(dt, *p.values(), B, L, C, n_images, max_len, seq_len, None)

    for f in (ctx_fwd, ctx_bwd):
        assert f(dt=9) == DTYPE and f(dt=3) == DTYPE
        assert f(max_len=0) == DIMS and f(max_len=-3) == DIMS and f(max_len=17) == DIMS       # < 1, > seq_len
        assert f(B=-1) == DIMS and f(L=-1) == DIMS and f(C=-8) == DIMS and f(n_images=-1) == DIMS
        assert f(C=12) == UNSUPPORTED and f(dt=0, C=6) == UNSUPPORTED
        assert f(row=None) == NULLPTR and f(col=None, start=None) == NULLPTR
    assert ctx_fwd(out=None) == NULLPTR and ctx_fwd(mask=None) == NULLPTR and ctx_fwd(src=None) == NULLPTR
    assert ctx_fwd(pos=odd) == ALIGN and ctx_fwd(bos=ctypes.c_void_p(4100)) == ALIGN
    assert ctx_fwd(n_images=0, out=None, mask=None) == 0
    assert ctx_bwd(grad=None) == NULLPTR and ctx_bwd(first=None) == NULLPTR and ctx_bwd(ws=None) == NULLPTR
    assert ctx_bwd(g_src=odd) == ALIGN and ctx_bwd(g_src=None, g_pad=None, grad=None) == 0

    ws = lib.mmfs_sequence_context_backward_workspace_bytes
    assert ws(2, 4096, 32) == 32 * 4096 * 4 and ws(0, 8, 0) == 0
    assert ws(3, 32, 4) == DTYPE and ws(2, 12, 4) == UNSUPPORTED and ws(2, 32, -1) == DIMS
