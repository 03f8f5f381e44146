"""The text loss's kernels (csrc/mmfs_text_loss.hip) on the device, through mmfs_amd.text_loss.

``loss``, ``lse``, the reduced loss and the gradient are held element by element to fp64 on the stored logits under the
bounds of the kernel file's header (tests/text_loss_refs.py states them); the framework route's fp32 result on the same
inputs is held to the SAME bounds, so a bound is one the reference statement itself meets.  Outputs are poisoned before
the kernels run: an element nobody wrote is NaN.

Worst bound ratios measured on an MI355X are kept in profiles/text_loss.md."""
import importlib

import pytest
import torch

from front_end_refs import worst
from helpers import poison_allocations
from text_loss_refs import classes, grad64, reduced64, rows64

tl = importlib.import_module("mmfs_amd.text_loss")

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
WIDTHS = [1, 2, 7, 8, 9, 511, 512, 513, 2049, 4099]


def func():
    from mmfs_amd.functions import text_loss_func
    return text_loss_func


def draw_logits(gen, shape, dtype, scale=4.0):
    return (torch.randn(*shape, generator=gen) * scale).to(DEV).to(dtype)


def placed_labels(gen, B, n, V):
    """labels at 0, at V - 1, at 1 (inside a peeled head) and at V - 2 (inside a tail), random ones, one row ignored"""
    labels = torch.randint(0, V, (B, n), generator=gen)
    flat = labels.view(-1)
    for k, v in enumerate((0, V - 1, min(1, V - 1), max(V - 2, 0))):
        flat[k % flat.numel()] = v
    flat[-1] = -100
    return labels.to(DEV)


def hold(what, got, ref, bound, report):
    w = worst(got.detach(), ref, bound)
    report.append((what, w[0]))
    assert w[0] <= 1.0, f"{what}: |got - ref| / bound = {w[0]:.3g} at {w[1]}: got {w[2]!r}, ref {w[3]!r}, bound {w[4]:.3g}"


def check_routes(x, labels, first, tag):
    """both routes on the same inputs against fp64 under the header's bounds; -> the worst ratios"""
    B, L, V = x.shape
    r = rows64(x, labels, first)
    n_valid = int(r["valid"].sum())
    report = []
    loss, lse, counts = func().row_losses(x, labels, first, -100)
    assert counts.tolist() == [n_valid, 0]
    hold(f"{tag} kernels lse", lse, r["lse"], r["E_lse"], report)
    hold(f"{tag} kernels loss", loss, r["loss"], r["E_loss"], report)
    for route in ("kernels", "framework"):
        leaf = x.clone().requires_grad_(True)
        before = func().launches["forward"], func().launches["backward"]
        rows = tl.text_loss(leaf, labels, reduction="none", first=first, route=route)
        mean = tl.text_loss(leaf, labels, first=first, route=route)
        assert rows.dtype == torch.float32 and rows.shape == labels.shape and mean.dtype == torch.float32 and mean.dim() == 0
        (grad,) = torch.autograd.grad(mean, leaf)
        took = func().launches["forward"] - before[0], func().launches["backward"] - before[1]
        assert took == ((2, 1) if route == "kernels" else (0, 0)), (route, took)
        assert grad.dtype == x.dtype and grad.shape == x.shape
        hold(f"{tag} {route} rows", rows, r["loss"], r["E_loss"], report)
        ref, bound = reduced64(r, "mean")
        hold(f"{tag} {route} mean", mean, ref, bound, report)
        g = torch.full(labels.shape, 1.0 / max(n_valid, 1), dtype=torch.float64, device=DEV)
        ref, bound = grad64(r, g, x.shape, first, x.dtype)
        hold(f"{tag} {route} grad", grad, ref, bound, report)
    return report


def show(report):
    by_kind = {}
    for what, ratio in report:
        kind = " ".join(what.split()[-2:])
        by_kind[kind] = max(by_kind.get(kind, 0.0), ratio)
    print("worst |got - ref| / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(by_kind.items())))


# ------------------------------------------------------------------ row geometry
@pytest.mark.parametrize("first", [0, 2])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
@pytest.mark.parametrize("V", WIDTHS)
def test_rows_of_every_geometry_hold_the_bounds(V, dtype, first, monkeypatch):
    """[B, L] = [2, 5]: with V odd every row starts on another boundary"""
    gen = torch.Generator().manual_seed(1000 * V + first)
    B, L = 2, 5
    x = draw_logits(gen, (B, L, V), dtype)
    labels = placed_labels(gen, B, L - 1 - first, V)
    poison_allocations(monkeypatch)
    show(check_routes(x, labels, first, f"V={V}"))


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
@pytest.mark.parametrize("shape", [(1, 9, 32003), (2, 3, 32002)], ids=lambda s: "x".join(map(str, s)))
def test_rows_of_the_real_width_hold_the_bounds(shape, dtype, monkeypatch):
    gen = torch.Generator().manual_seed(shape[2])
    x = draw_logits(gen, shape, dtype)
    labels = placed_labels(gen, shape[0], shape[1] - 1, shape[2])
    poison_allocations(monkeypatch)
    show(check_routes(x, labels, 0, f"V={shape[2]}"))


def test_none_and_sum_gradients_hold_the_bounds(monkeypatch):
    """the other two reductions: a row's own upstream, and the scalar's"""
    gen = torch.Generator().manual_seed(7)
    B, L, V, first, dtype = 2, 6, 513, 1, torch.bfloat16
    x = draw_logits(gen, (B, L, V), dtype)
    labels = placed_labels(gen, B, 4, V)
    up = torch.randn(B, 4, generator=gen).to(DEV)
    poison_allocations(monkeypatch)
    r = rows64(x, labels, first)
    report = []
    for route in ("kernels", "framework"):
        leaf = x.clone().requires_grad_(True)
        rows = tl.text_loss(leaf, labels, reduction="none", first=first, route=route)
        (grad,) = torch.autograd.grad(rows, leaf, up)
        ref, bound = grad64(r, up.double(), x.shape, first, dtype)
        hold(f"{route} none grad", grad, ref, bound, report)
        total = tl.text_loss(leaf, labels, reduction="sum", first=first, route=route)
        ref, bound = reduced64(r, "sum")
        hold(f"{route} sum sum", total, ref, bound, report)
        (grad,) = torch.autograd.grad(total, leaf, torch.tensor(-1.5, device=DEV))
        ref, bound = grad64(r, torch.full((B, 4), -1.5, dtype=torch.float64, device=DEV), x.shape, first, dtype)
        hold(f"{route} sum grad", grad, ref, bound, report)
    show(report)


# ------------------------------------------------------------------ exact zeros, reproducibility
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
def test_unscored_rows_are_zero_bits_and_two_runs_agree_bit_for_bit(dtype, monkeypatch):
    gen = torch.Generator().manual_seed(11)
    B, L, V, first, n = 2, 6, 513, 1, 4                         # rows 0 and 5 lie outside the window
    x = draw_logits(gen, (B, L, V), dtype)
    labels = placed_labels(gen, B, n, V)
    labels[0, 2] = -100
    poison_allocations(monkeypatch)
    bits = {torch.float32: torch.int32}.get(dtype, torch.int16)

    def run():
        leaf = x.clone().requires_grad_(True)
        loss, lse, counts = func().row_losses(leaf.detach(), labels, first, -100)
        mean = tl.text_loss(leaf, labels, first=first, route="kernels")
        (grad,) = torch.autograd.grad(mean, leaf)
        return loss, lse, counts, mean, grad

    a, b = run(), run()
    raw = lambda t: t.reshape(-1).contiguous().view(torch.uint8)
    for name, u, v in zip(("loss", "lse", "counts", "mean", "grad"), a, b):
        assert torch.equal(raw(u), raw(v)), name
    grad = a[4].view(bits)
    zero_rows = torch.ones(B, L, dtype=torch.bool, device=DEV)
    zero_rows[:, first:first + n] = labels == -100
    assert int(zero_rows.sum()) == 2 * 2 + 2
    assert not bool(grad[zero_rows].any()), "an unscored row holds a bit"
    assert bool((grad[~zero_rows] != 0).any(-1).all())
    # training's window: the last position is never scored
    leaf = x.clone().requires_grad_(True)
    full = placed_labels(gen, B, L - 1, V)
    (grad,) = torch.autograd.grad(tl.text_loss(leaf, full, route="kernels"), leaf)
    assert not bool(grad[:, -1].view(bits).any()) and not bool(grad[1, L - 2].view(bits).any())


# ------------------------------------------------------------------ non-finite logits
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=lambda d: str(d).split(".")[1])
def test_non_finite_logits_fall_where_the_framework_has_them(dtype, monkeypatch):
    """row 0: scattered -Inf; 1: the first 4096 entries -Inf; 2: all -Inf; 3: one +Inf; 4: one NaN"""
    gen = torch.Generator().manual_seed(13)
    B, L, V = 1, 6, 8203
    x = draw_logits(gen, (B, L, V), dtype)
    inf = float("inf")
    x[0, 0, torch.randint(0, V, (600,), generator=gen).to(DEV)] = -inf
    x[0, 1, :4096] = -inf
    x[0, 2] = -inf
    x[0, 3, 5000] = inf
    x[0, 4, 17] = float("nan")
    labels = torch.tensor([[4100, 8000, 3, 9, 100]], device=DEV)
    x[0, 0, 4100] = 1.0                                         # (the scored entries of rows 0 and 1 are finite)
    poison_allocations(monkeypatch)
    out = {}
    for route in ("kernels", "framework"):
        leaf = x.clone().requires_grad_(True)
        rows = tl.text_loss(leaf, labels, reduction="none", route=route)
        (grad,) = torch.autograd.grad(rows, leaf, torch.ones_like(rows))
        out[route] = rows.double(), grad.double()
    for k, f, name in zip(out["kernels"], out["framework"], ("loss", "grad")):
        assert torch.equal(torch.isnan(k), torch.isnan(f)), name
        assert torch.equal(torch.isinf(k), torch.isinf(f)) and torch.equal(k[torch.isinf(k)], f[torch.isinf(f)]), name
    assert bool(torch.isfinite(out["framework"][0][0, :2]).all()) and bool(torch.isnan(out["kernels"][0][0, 2:]).all())
    # the finite rows against fp64 under the bounds
    r = rows64(x[:, :2], labels[:, :2], 0)
    report = []
    hold("loss", out["kernels"][0][:, :2], r["loss"], r["E_loss"], report)
    ref, bound = grad64(r, torch.ones(1, 2, dtype=torch.float64, device=DEV), (1, 2, V), 0, dtype)
    hold("grad", out["kernels"][1][:, :2], ref, bound, report)
    hold("framework grad", out["framework"][1][:, :2], ref, bound, report)
    assert not bool(out["kernels"][1][0, 5].any())
    show(report)


# ------------------------------------------------------------------ ignored and out-of-range labels
def test_every_label_ignored_is_nan_with_zero_gradient_on_both_routes(monkeypatch):
    gen = torch.Generator().manual_seed(17)
    x = draw_logits(gen, (2, 5, 513), torch.bfloat16)
    labels = torch.full((2, 4), -100, device=DEV)
    poison_allocations(monkeypatch)
    for route in ("kernels", "framework"):
        leaf = x.clone().requires_grad_(True)
        mean = tl.text_loss(leaf, labels, route=route)
        (grad,) = torch.autograd.grad(mean, leaf)
        assert bool(torch.isnan(mean)), route
        assert not bool(grad.view(torch.int16).any()), route
        assert float(tl.text_loss(x, labels, reduction="sum", route=route)) == 0.0


def test_out_of_range_labels_are_counted_never_read_and_validate_raises(monkeypatch):
    gen = torch.Generator().manual_seed(19)
    B, L, V = 2, 6, 513
    x = draw_logits(gen, (B, L, V), torch.bfloat16)
    clean = placed_labels(gen, B, L - 1, V)
    labels = clean.clone()
    labels[0, 1], labels[1, 0], labels[1, 2] = -1, V, 1 << 40
    as_ignored = labels.clone()
    as_ignored[(labels < 0) | (labels >= V)] = -100
    assert classes(labels, V, -100)[1].sum() == 3
    poison_allocations(monkeypatch)
    loss, lse, counts = func().row_losses(x, labels, 0, -100)
    want = func().row_losses(x, as_ignored, 0, -100)
    assert counts.tolist() == [int((as_ignored != -100).sum()), 3] and want[2].tolist() == [counts[0].item(), 0]
    assert torch.equal(loss, want[0]) and torch.equal(lse, want[1])
    assert not bool(loss[as_ignored == -100].any())
    for route in ("kernels", "framework"):
        leaf = x.clone().requires_grad_(True)
        ref_leaf = x.clone().requires_grad_(True)
        got = tl.text_loss(leaf, labels, route=route)
        ref = tl.text_loss(ref_leaf, as_ignored, route=route, validate=True)
        assert torch.equal(got, ref) and bool(torch.isfinite(got))
        assert torch.equal(torch.autograd.grad(got, leaf)[0], torch.autograd.grad(ref, ref_leaf)[0])
        with pytest.raises(IndexError):
            tl.text_loss(x, labels, route=route, validate=True)


# ------------------------------------------------------------------ no host round trip
def test_forward_and_backward_are_captured_and_replayed():
    """forward + backward in ONE graph on one stream; logits and labels are rewritten in place so that the number of valid
    rows changes, and the replay equals the eager call on the new inputs bit for bit.  A sync inside would have failed the
    capture."""
    gen = torch.Generator().manual_seed(23)
    B, L, V, dtype = 2, 7, 4099, torch.bfloat16
    x = draw_logits(gen, (B, L, V), dtype)
    labels = placed_labels(gen, B, L - 1, V)
    second = placed_labels(gen, B, L - 1, V)
    second[0, :3] = -100
    assert int((second != -100).sum()) != int((labels != -100).sum())

    def step():
        leaf = x.detach().requires_grad_(True)                   # (a leaf of this call, on the storage that is rewritten)
        mean = tl.text_loss(leaf, labels, route="kernels")
        (grad,) = torch.autograd.grad(mean, leaf)
        return mean.detach(), grad

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    x.copy_(draw_logits(gen, (B, L, V), dtype))
    labels.copy_(second)
    graph.replay()
    torch.cuda.synchronize()
    got = [t.clone() for t in captured]
    want = step()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(want[0])) and torch.equal(got[0], want[0])
    assert torch.equal(got[1].view(torch.int16), want[1].view(torch.int16))
    r = rows64(x, labels, 0)
    ref, bound = reduced64(r, "mean")
    assert worst(got[0], ref, bound)[0] <= 1.0


# ------------------------------------------------------------------ beyond 2^31 elements
def test_rows_behind_2_to_the_31_elements(monkeypatch):
    """bf16 logits [1, 67200, 32003]: 2.15 * 10^9 elements (4.3 GB, and a gradient as large); 64 rows at the start and 64 at
    the end are scored through ``first``, in two calls, against the framework route on those slices."""
    B, L, V, n = 1, 67200, 32003, 64
    assert B * L * V > 1 << 31
    gen = torch.Generator(device=DEV).manual_seed(29)
    x = torch.empty((B, L, V), dtype=torch.bfloat16, device=DEV)
    x.normal_(0.0, 4.0, generator=gen)
    cpu = torch.Generator().manual_seed(31)
    labels = placed_labels(cpu, B, n, V)
    poison_allocations(monkeypatch)
    for first in (0, L - n):
        leaf = x.requires_grad_(True)
        mean = tl.text_loss(leaf, labels, first=first, route="kernels")
        (grad,) = torch.autograd.grad(mean, leaf)
        piece = x.detach()[:, first:first + n].clone().requires_grad_(True)
        want = tl.text_loss(piece, labels, route="framework")
        (want_grad,) = torch.autograd.grad(want, piece)
        r = rows64(piece.detach(), labels, 0)
        ref, bound = reduced64(r, "mean")
        assert worst(mean.detach(), ref, bound)[0] <= 1.0 and worst(want.detach(), ref, bound)[0] <= 1.0, first
        g = torch.full((B, n), 1.0 / int(r["valid"].sum()), dtype=torch.float64, device=DEV)
        ref, bound = grad64(r, g, (B, n, V), 0, torch.bfloat16)
        w = worst(grad[:, first:first + n], ref, bound)
        assert w[0] <= 1.0, (first, w)
        assert worst(want_grad, ref, bound)[0] <= 1.0, first
        outside = grad[:, n:] if first == 0 else grad[:, :first]
        assert not bool(outside.view(torch.int16).any()), first
        del grad, outside, mean


# ------------------------------------------------------------------ option scores
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
def test_option_scores_agree_with_the_framework_route(dtype, monkeypatch):
    gen = torch.Generator().manual_seed(37)
    n_options, L, V, n, context_offset = 3, 12, 4099, 5, 6
    x = draw_logits(gen, (n_options, L, V), dtype)
    ids = torch.randint(0, V, (n_options, n), generator=gen).to(DEV)
    mask = torch.ones(n_options, n, dtype=torch.long, device=DEV)
    mask[1, 3:] = 0
    mask[2, 1:] = 0
    poison_allocations(monkeypatch)
    got = tl.option_scores(x, ids, mask, context_offset=context_offset, route="kernels")
    want = tl.option_scores(x, ids, mask, context_offset=context_offset, route="framework")
    assert got.shape == (n_options,) and got.dtype == torch.float32 and not got.requires_grad
    r = rows64(x, ids, context_offset - 1, ignore_index=-(1 << 63))
    ref = -(r["loss"] * mask).sum(-1)
    # the row bound of each unmasked token, and the fp32 sum of at most n terms
    bound = (r["E_loss"] * mask).sum(-1) + n * 2.0 ** -24 * (r["loss"].abs() * mask).sum(-1)
    for name, t in (("kernels", got), ("framework", want)):
        w = worst(t, ref, bound)
        assert w[0] <= 1.0, (name, w)
