"""The interleaved sequence's kernels (csrc/mmfs_sequence.hip) on the device, through mmfs_amd.sequence.

Copies and single roundings (the tables, the forwards, the mask, grad_text, grad_vis) are held bit for bit to the
framework route on the same inputs.  Sums are held to fp64 under the bound of the kernel file's header,

    |got - want| <= u_T |want| + t_T + (n - 1) 2^-24 sum |terms|          n: the header's chain for that element

and the projected features to the reference's fp64 fixture under front_end_refs.linear_bounds plus the roundings of the
inputs, the table and the last add (derived where it is built).  Outputs are poisoned before the kernels run: an
element nobody wrote is NaN."""
import pytest
import torch

from front_end_refs import E24, linear64, linear_bounds, worst
from helpers import STORAGE_T, STORAGE_U, poison_allocations
from test_sequence import (assert_tables, context_call, embed_call, fixture, index_layouts, projection)

from mmfs_amd import sequence as seq

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
WIDTHS = ["one_vector", "three_vectors", "136"]


def width(kind, dtype):
    vec = 16 // torch.empty(0, dtype=dtype).element_size()
    return {"one_vector": vec, "three_vectors": 3 * vec, "136": 136}[kind]


def counts_of(ids, image_id, soi_id):
    return int((ids == image_id).sum()), int((ids == soi_id).sum())


# ------------------------------------------------------------------ the tables
@pytest.mark.parametrize("layout", index_layouts(), ids=lambda l: l[0])
def test_index_kernel_matches_the_host(layout, monkeypatch):
    from mmfs_amd.functions import sequence_func
    _, ids, image_id, soi_id = layout
    n_img, n_soi = counts_of(ids, image_id, soi_id)
    poison_allocations(monkeypatch)
    for n_vis, n_images in ((n_img, n_soi), (n_img + 1, n_soi + 1), (max(n_img - 1, 0), max(n_soi - 1, 0))):
        before = sequence_func.launches["index"]
        t = seq.sequence_tables(ids.to(DEV), image_token_id=image_id, soi_token_id=soi_id, n_vis=n_vis, n_images=n_images,
                                route="kernels")
        assert sequence_func.launches["index"] == before + 1
        assert_tables(t, ids, image_id, soi_id, n_vis, n_images)
        f = seq.sequence_tables(ids.to(DEV), image_token_id=image_id, soi_token_id=soi_id, n_vis=n_vis, n_images=n_images,
                                route="framework")
        assert all(torch.equal(a, b) for a, b in zip(t[:6], f[:6]))


# ------------------------------------------------------------------ the embeddings
@pytest.mark.parametrize("text_fp32", [False, True], ids=["text_T", "text_fp32"])
@pytest.mark.parametrize("kind", WIDTHS)
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_embed_kernels(dtype, kind, text_fp32, monkeypatch):
    C = width(kind, dtype)
    gen = torch.Generator().manual_seed(11)
    u, t = STORAGE_U[dtype], STORAGE_T[dtype]
    for name, ids, image_id, soi_id in index_layouts():
        B, L = ids.shape
        n_img, n_soi = counts_of(ids, image_id, soi_id)
        for n_vis in sorted({n_img, n_img + 1, max(n_img - 1, 0)}):
            draw = lambda *s: torch.randn(*s, generator=gen).to(DEV)
            text = draw(B, L, C).to(torch.float32 if text_fp32 else dtype)
            vis, soi, grad = draw(n_vis, C).to(dtype), draw(1, C).to(dtype), draw(B, L, C).to(dtype)
            g = dict(text_ids=ids.to(DEV), image_id=image_id, soi_id=soi_id)

            def run(route):
                leaves = [x.clone().requires_grad_(True) for x in (text, vis, soi)]
                out = embed_call(g, *leaves, route=route)
                grads = torch.autograd.grad(out, leaves, grad, allow_unused=True)      # (no visual row: vis is not read)
                return (out.detach(),) + tuple(torch.zeros_like(x) if v is None else v for v, x in zip(grads, leaves))

            want = run("framework")
            with monkeypatch.context() as m:
                poison_allocations(m)
                got = run("kernels")
            where = (name, n_vis)
            assert got[0].dtype == dtype and got[1].dtype == text.dtype
            for what, a, b in zip(("out", "grad_text", "grad_vis"), got[:3], want[:3]):
                assert torch.equal(a, b), (what,) + where
            # grad_soi: the <soi> rows in ascending order, fp32, one rounding: n = their number
            rows = grad.reshape(B * L, C)[(ids.reshape(-1) == soi_id).to(DEV)].double()
            ref, terms = rows.sum(0, keepdim=True), rows.abs().sum(0, keepdim=True)
            bound = u * ref.abs() + t + max(n_soi - 1, 0) * E24 * terms
            w = worst(got[3], ref, bound)
            print(f"grad_soi {dtype} C={C} {where}: n={n_soi} worst ratio {w[0]:.3f}")
            assert w[0] <= 1.0, (where, w)


# ------------------------------------------------------------------ the context gather
def b2_layout():
    """B = 2, L = 40: three images in row 0 (<soi> at column 0, two sharing context), two in row 1 (one at L - 1); image 2
    has its <bos> behind its <soi> (no context at all).  Lengths [1, 8, 0, 18, 35]."""
    gen = torch.Generator().manual_seed(23)
    ids = torch.randint(10, 50, (2, 40), generator=gen)
    for r, c in ((0, 0), (0, 10), (0, 25), (1, 17), (1, 39)):
        ids[r, c] = 5
    return ids, torch.tensor([0, 3, 30, 0, 5]), 35


def golden_layout():
    g = fixture("sequence_bos")
    return g["text_ids"], g["nearest_bos_idxs"], 24


def gather64(P, pad, pos, tables, bos, max_len):
    """the framework statement in fp64 with autograd -> out, and the leaves"""
    P64 = P.double().requires_grad_(True)
    pad64 = None if pad is None else pad.double().requires_grad_(True)
    out, mask = seq._gather_framework(P64, pad64, None if pos is None else pos.double(), tables, None, bos, max_len)
    return out, mask, P64, pad64


@pytest.mark.parametrize("extra_slot", [0, 1], ids=["slots_exact", "one_slot_more"])
@pytest.mark.parametrize("kind", ["golden_C16"] + WIDTHS)
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_context_gather_kernels(dtype, kind, extra_slot, monkeypatch):
    ids, bos, longest = golden_layout() if kind == "golden_C16" else b2_layout()
    C = 16 if kind == "golden_C16" else width(kind, dtype)
    B, L = ids.shape
    soi_id = 60 if kind == "golden_C16" else 5
    n_images = int((ids == soi_id).sum()) + extra_slot
    bos = torch.cat((bos, bos.new_zeros(extra_slot))).to(DEV)
    seq_len = L + 8
    u, t = STORAGE_U[dtype], STORAGE_T[dtype]
    gen = torch.Generator().manual_seed(31)
    draw = lambda *s: torch.randn(*s, generator=gen).to(DEV).to(dtype)
    tables = seq.sequence_tables(ids.to(DEV), image_token_id=-1, soi_token_id=soi_id, n_vis=0, n_images=n_images)
    lengths = seq._windows(tables, None, bos, L, L)[2]
    assert int(lengths.max()) == longest
    for max_len in (longest - 4, longest, longest + 5):                  # cut, exact, padding behind every image
        for with_pad_pos in (True, False):
            P, grad = draw(B, L, C), draw(n_images, max_len, C)
            pad = draw(C) if with_pad_pos else None
            pos = draw(seq_len, C) if with_pad_pos else None
            where = (kind, max_len, with_pad_pos)

            def run(route):
                leaves = [P.clone().requires_grad_(True)] + ([pad.clone().requires_grad_(True)] if with_pad_pos else [])
                out, mask = seq._gather(leaves[0], leaves[1] if with_pad_pos else None, pos, tables, None, bos, max_len,
                                        route, "test")
                return (out.detach(), mask) + torch.autograd.grad(out, leaves, grad)

            want = run("framework")
            with monkeypatch.context() as m:
                poison_allocations(m)
                got = run("kernels")
            assert got[0].dtype == dtype and got[1].dtype == torch.long
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), where
            assert got[1].sum(1).tolist() == lengths.clamp_max(max_len).tolist()
            # gradients against fp64: the terms of an element are the gradient rows that read it; their number and the
            # sum of their magnitudes come from the same fp64 statement run on ones and on |grad|
            out64, _, P64, pad64 = gather64(P, pad, pos, tables, bos, max_len)
            leaves64 = [P64] + ([pad64] if with_pad_pos else [])
            ref = torch.autograd.grad(out64, leaves64, grad.double(), retain_graph=True)
            mags = torch.autograd.grad(out64, leaves64, grad.double().abs(), retain_graph=True)
            cnt = torch.autograd.grad(out64, leaves64, torch.ones_like(out64))
            n_src = cnt[0].amax(-1, keepdim=True)                        # covering images per token
            bound = u * ref[0].abs() + t * (n_src > 0) + (n_src - 1).clamp_min(0) * E24 * mags[0]
            w = worst(got[2], ref[0], bound)
            print(f"grad_src {dtype} C={C} {where}: worst ratio {w[0]:.3f}")
            assert w[0] <= 1.0, (where, w)
            if with_pad_pos:
                # the header's rule: stage 1 adds an image's padded rows, stage 2 the images
                n_pad = int((max_len - lengths.clamp_max(max_len)).max()) + n_images - 1
                bound = u * ref[1].abs() + t + max(n_pad - 1, 0) * E24 * mags[1]
                w = worst(got[3], ref[1], bound)
                print(f"grad_pad {dtype} C={C} {where}: n={n_pad} worst ratio {w[0]:.3f}")
                assert w[0] <= 1.0, (where, w)


@pytest.mark.parametrize("order", ["project_first", "gather_first"])
@pytest.mark.parametrize("case", ["sequence_bos", "sequence_start"])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_projected_context_against_the_fixture(dtype, case, order, monkeypatch):
    """Both orders, kernels on, against the reference's fp64 features.  Per element, with y = the fp64 projection of the
    token (the bias alone for a padded row) and s = sum |x w| + |b|:
        linear_bounds(y, s, K, T)          the product in T: fp32 sums, one rounding (front_end_refs)
      + (2 u + u^2) (s - |b|) + u |b|      16-bit only: x, W and b are the fixture's fp32 draws ROUNDED to T
      + u |pos|                            16-bit only: the table is rounded to T before it is added
      + u |y + pos| + t                    the add's own rounding
    the rounded-input lines times (1 + u): the later roundings act on the values they have shifted
    (fp32: the fixture's inputs and table are exact in T and the middle lines vanish)."""
    from mmfs_amd.functions import sequence_func
    g = fixture(case)
    u, t = STORAGE_U[dtype], STORAGE_T[dtype]
    x = g["context_features"].to(DEV, dtype)
    proj = projection(g, dtype, DEV)
    before = dict(sequence_func.launches)
    with torch.no_grad(), monkeypatch.context() as m:
        poison_allocations(m)
        feats, mask = context_call(g, x, proj, order=order, route="kernels")
    assert sequence_func.launches["context_forward"] == before["context_forward"] + 1
    assert feats.dtype == dtype and torch.equal(mask.cpu(), g["mask"])
    K = x.shape[-1]
    y, s = linear64(g["context_features"].reshape(-1, K), g["weight"], g["bias"])
    b_abs = g["bias"].abs()
    rounded = 0.0 if dtype == torch.float32 else 1.0
    tok = linear_bounds(y, s, K, dtype) + rounded * (1 + u) * ((2 * u + u * u) * (s - b_abs) + u * b_abs)
    pad = linear_bounds(g["bias"], b_abs, K, dtype) + rounded * (1 + u) * u * b_abs
    tables = seq.sequence_tables(g["text_ids"], image_token_id=-1, soi_token_id=g["soi_id"], n_vis=0, n_images=4)
    per_image, _ = seq._gather_framework(tok.view(3, 24, K), pad, None, tables, g.get("image_start_token_idx"),
                                         g.get("nearest_bos_idxs"), 24)
    pos = g["pos_table"].double()[:24]
    bound = (1 + u) * (per_image + rounded * u * pos.abs()) + u * g["features"].abs() + t
    w = worst(feats.cpu(), g["features"], bound)
    print(f"features {dtype} {case} {order}: worst ratio {w[0]:.3f}")
    assert w[0] <= 1.0, w


def test_context_gradients_through_the_module_against_the_fixture(monkeypatch):
    """fp32, project_first, kernels on: the gradients of the context, the weight and the bias (real rows through
    F.linear, padded rows through the gather) against the fixture's.  Each is a sum of at most n_images L = 96 (context),
    B L + 96 = 168 (weight, bias) products of fp32 numbers: (n + 1) 2^-24 sum |terms|, the sum of magnitudes bounded by
    n max|a| max|b| -- a loose, order-free bound; its point is the route, the tight ones are above."""
    g = fixture("sequence_bos")
    x = g["context_features"].to(DEV, torch.float32).requires_grad_(True)
    proj = projection(g, torch.float32, DEV)
    with monkeypatch.context() as m:
        poison_allocations(m)
        feats, _ = context_call(g, x, proj, order="project_first", route="kernels")
        feats.backward(g["grad_out.features"].to(DEV, torch.float32))
    gmax = float(g["grad_out.features"].abs().max())
    for name, leaf, n, other in (("context_features", x, 96 * 16, float(g["weight"].abs().max())),
                                 ("weight", proj.weight, 168, float(g["context_features"].abs().max())),
                                 ("bias", proj.bias, 168, 1.0)):
        bound = torch.full_like(g["grad." + name], (n + 1) * E24 * n * gmax * other)
        w = worst(leaf.grad.cpu(), g["grad." + name], bound)
        print(f"grad {name}: worst ratio {w[0]:.3g}")
        assert w[0] <= 1.0, (name, w)


# ------------------------------------------------------------------ no host round trip
def test_the_whole_sequence_is_captured_and_replayed():
    """tables + embeddings + context (max_len given, no validation) in ONE graph on one stream; text_ids and the inputs
    are rewritten in place and the replay equals the eager call on the new inputs bit for bit.  A sync inside would have
    failed the capture."""
    dtype, B, L, C, n_vis, n_images, max_len, seq_len = torch.bfloat16, 2, 40, 136, 6, 6, 24, 48
    gen = torch.Generator().manual_seed(47)
    draw = lambda *s: torch.randn(*s, generator=gen).to(DEV).to(dtype)

    def layout(soi_at, image_at):
        ids = torch.randint(10, 50, (B, L), generator=gen)
        for r, c in soi_at:
            ids[r, c] = 5
        for r, c in image_at:
            ids[r, c] = 4
        return ids.to(DEV)

    first = layout(((0, 0), (0, 10), (0, 25), (1, 17), (1, 39)), ((0, 1), (0, 2), (0, 11), (0, 26), (1, 18), (1, 19)))
    second = layout(((0, 39), (1, 0), (1, 5)), ((0, 3), (1, 1), (1, 6), (1, 7)))
    ids, bos = first.clone(), torch.tensor([0, 3, 30, 0, 5, 0], device=DEV)
    text, vis, soi, ctx = draw(B, L, C), draw(n_vis, C), draw(1, C), draw(B, L, C)
    torch.manual_seed(48)
    proj = torch.nn.Linear(C, C).to(DEV, dtype)

    def step():
        with torch.no_grad():
            tables = seq.sequence_tables(ids, image_token_id=4, soi_token_id=5, n_vis=n_vis, n_images=n_images, route="kernels")
            mm = seq.assemble_mm_embeds(text, ids, vis, soi, image_token_id=4, soi_token_id=5, tables=tables, route="kernels")
            feats, mask = seq.prepare_context_features_for_image_decoder(
                ctx, ids, proj, soi_token_id=5, n_images=n_images, seq_len=seq_len, nearest_bos_idxs=bos, max_len=max_len,
                order="project_first", tables=tables, route="kernels")
        return mm, feats, mask

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                   # (the kept sin-cos table and the BLAS workspace exist now)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    ids.copy_(second)
    bos.copy_(torch.tensor([2, 0, 1, 0, 0, 0], device=DEV))
    for x in (text, vis, soi, ctx):
        x.copy_(draw(*x.shape))
    graph.replay()
    torch.cuda.synchronize()
    got = [x.clone() for x in captured]
    want = step()
    torch.cuda.synchronize()
    assert int(want[2].sum()) > 0 and bool(torch.isfinite(want[1].float()).all())
    for name, a, b in zip(("mm_embeds", "features", "mask"), got, want):
        assert torch.equal(a, b), name
