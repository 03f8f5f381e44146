"""Shared test helpers: seeded inputs in the reference's test distribution
(ops/tests/create_data.py:11-30) and golden loading."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mm-interleaved_amd")
LIB = os.path.join(PKG, "libmmfs_msda.so")


def bound_library():
    """A ``ctypes.CDLL`` handle of the caller's own on the kernel library, every entry point of include/mmfs_msda.h bound
    by the package's one signature table (mmfs_abi.py)."""
    import ctypes
    import mmfs_abi                                        # (beside the shim; conftest.py puts that directory on sys.path)
    assert os.path.exists(LIB), "run __graft_entry__.build() / make -C mm-interleaved_amd/csrc"
    return mmfs_abi.bind(ctypes.CDLL(LIB))


def load_golden(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))


def level_tables(shapes, device="cpu"):
    sh = torch.as_tensor(shapes, dtype=torch.long, device=device).reshape(-1, 2)
    start = torch.cat((sh.new_zeros(1), sh.prod(1).cumsum(0)[:-1]))
    return sh.contiguous(), start.contiguous()


def make_inputs(B, H, D, Nq, P, shapes, seed=0, loc_range=(0.0, 1.0), dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    sh, start = level_tables(shapes)
    S, L = int(sh.prod(1).sum()), sh.shape[0]
    value = torch.rand(B, S, H, D, generator=g)
    lo, hi = loc_range
    loc = torch.rand(B, Nq, H, L, P, 2, generator=g) * (hi - lo) + lo
    attn = torch.rand(B, Nq, H, L, P, generator=g) + 1e-5
    attn = attn / attn.sum(-1, keepdim=True).sum(-2, keepdim=True)
    grad = torch.randn(B, Nq, H * D, generator=g)
    # round through the storage dtype so oracle and device see identical numbers
    rt = lambda t: t.to(dtype).to(torch.float64)
    return dict(value=rt(value), shapes=sh, start=start, loc=rt(loc), attn=rt(attn), grad=rt(grad))


def poison(t):
    """Fill a freshly allocated tensor so that an element nobody writes cannot pass for a result: NaN for floating types
    (0xff bytes for the one-byte floats), 0xA5 bytes for uint8 workspaces, True for bool, 0x5A5A... for the other
    integer types.  -> t."""
    if t.numel() == 0 or t.device.type == "meta":
        return t
    with torch.no_grad():                      # (an allocation may ask for requires_grad)
        _fill_poison(t)
    return t


def _fill_poison(t):
    if t.is_floating_point() or t.is_complex():
        if t.element_size() == 1:
            t.view(torch.uint8).fill_(0xFF)
        else:
            t.fill_(float("nan"))
    elif t.dtype == torch.uint8:
        t.fill_(0xA5)
    elif t.dtype == torch.bool:
        t.fill_(True)
    else:
        t.fill_(int.from_bytes(b"\x5a" * t.element_size(), "little"))


def poison_allocations(monkeypatch):
    """For the rest of a test: torch.empty / torch.empty_like hand out poisoned tensors (every argument passed through).
    The caching allocator often returns the block the previous identical call just freed -- and that block holds the
    previous call's answer, so an output element a kernel never writes would pass; under this it is NaN (or a pattern)."""
    empty, empty_like = torch.empty, torch.empty_like
    monkeypatch.setattr(torch, "empty", lambda *a, **k: poison(empty(*a, **k)))
    monkeypatch.setattr(torch, "empty_like", lambda *a, **k: poison(empty_like(*a, **k)))


def max_abs(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64).reshape(a.shape)
    return float(np.max(np.abs(a - b))) if a.size else 0.0


# ---------------------------------------------------------------------------------------------------------------------
# Per-element error bound of the op's outputs against the fp64 oracle.
#
# A bar relative to the LARGEST reference entry (TOL * max|ref|) leaves the small entries unconstrained: for bf16 it is
# larger than a whole grad_value entry at a third of the touched pixels, so a dropped, misrouted or stray contribution
# passes.  Here every element e has its own bound
#
#     |got_e - ref_e| <= u_s |ref_e| + t_s [A_e > 0] + gamma A_e + sum_l lam_l A'_{e,l} (+ w_s A''_e)
#
#   u_s    the storage type's rounding of the result (one rounding at the end) -- relative for normal numbers; below
#          the smallest normal number the rounding is absolute, half the subnormal spacing (t_s: 2^-25 for fp16, whose
#          grad_value entries of ~1e-5 are subnormal), added where A_e > 0.
#   A_e    the sum of the absolute values of the terms that make up e (exact, from the oracle on |inputs|; for grad_loc,
#          whose derivative weights carry signs, attn * extent * sum_c |g_c| * sum_corners |v_c| with unit weights).
#   gamma  covers the products and the fp32 sums.  The kernels carry every weight the matrix cores see as hi + lo 16-bit
#          parts (>= 16 significant bits: <= 2^-16 relative per weight, csrc/msda_bwd_tile.hip, msda_fwd_mma.hip,
#          msda_fwd_q8.hip, msda_fwd_wq.hip, msda_dense.hip), and a term is a product of <= 4 fp32 factors (weight,
#          attention, value, grad: <= 4 * 2^-24 more).  Sums are fp32 with one rounding at the end; an fp32 sum of n
#          terms is off by <= (n - 1) 2^-24 A in the worst case, ~2^-24 sqrt(n / 3) A when the partial sums grow
#          steadily (all terms one sign: the forward on positive maps), ~2^-24 A when the signs are mixed (grad_value,
#          grad_attn, grad_loc: the partial sums of a random walk stay far below A).  So 16-bit storage:
#          2^-16 + 2^-22 + (fp32 sums, < 2^-16 up to n = 256) < 2^-15, taken as 2^-14 (a factor 2 of margin for the
#          worst of ~10^6 elements; fp32 / fp16 storage keeps more bits of the weight than this).  fp32 storage (no
#          hi + lo split; the vector ALUs multiply in fp32): 4 * 2^-24 per term + 2^-24 sqrt(n / 3) for the sums at
#          n <= 1000 samples of a forward element, 2^-24 (4 + 18) < 2^-19.5, taken as 2^-19.  fp64: the same count at
#          2^-53 for <= 2^8 ulps of 2^-53: 2^-45.  Ceilings: 2^-12 (16-bit), 2^-18 (fp32).
#   lam_l  covers the bilinear weights, computed in fp32 from loc * extent - 0.5: an absolute error of <= 2^-24 extent
#          in the coordinate (the product) and as much again in the subtraction and 1 - f, so <= 2^-23 max(H_l, W_l) on
#          each weight; A'_{e,l} is A_e's sum over the samples of level l with every bilinear weight replaced by 1.
#          (Without it the oracle's own fp32 evaluation breaks the bound by ~19x on 40-pixel-wide levels; with it the
#          worst ratio is ~0.3: tests/test_error_bounds.py.)  fp64 arithmetic: 2^-52 max(H_l, W_l).
#   w_s    fp16 storage only: the matrix-core routes carry a weight as fp16 hi + lo parts, and below ~2^-3 the lo part
#          lies in fp16's subnormal range, so the weight is off by up to one subnormal spacing, 2^-24, absolute (not
#          2^-16 relative).  Each term then adds <= 2^-24 times its other factors: w_s A''_e, A'' being A with every
#          bilinear and attention weight replaced by 1 (out, grad_value, grad_attn).  Seen on the GPU as grad_value
#          errors of 1-2 subnormal spacings on entries of ~1e-6; bf16 has fp32's exponent range and no such term.
#
# Where all inputs are finite and A_e == 0 (untouched pixels, samples wholly outside the map), the bound is 0: the
# element must be exactly 0.
# ---------------------------------------------------------------------------------------------------------------------
OUTPUTS = ("out", "grad_value", "grad_loc", "grad_attn")
STORAGE_U = {torch.float64: 2.0 ** -53, torch.float32: 2.0 ** -24, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
STORAGE_T = {torch.float64: 2.0 ** -1075, torch.float32: 2.0 ** -150, torch.float16: 2.0 ** -25, torch.bfloat16: 2.0 ** -134}
GAMMA = {torch.float64: 2.0 ** -45, torch.float32: 2.0 ** -19, torch.float16: 2.0 ** -14, torch.bfloat16: 2.0 ** -14}
GAMMA_CEILING = {torch.float64: 2.0 ** -40, torch.float32: 2.0 ** -18, torch.float16: 2.0 ** -12, torch.bfloat16: 2.0 ** -12}
LAM_ULP = {torch.float64: 2.0 ** -52, torch.float32: 2.0 ** -23, torch.float16: 2.0 ** -23, torch.bfloat16: 2.0 ** -23}
HALF_WEIGHT_FLOOR = 2.0 ** -24     # w_s: an fp16 weight's lo part in the subnormal range
NEAR_CROSSING = 1e-4        # grad_loc jumps where a pixel coordinate crosses an integer: samples this close are left out


def level_lams(shapes, dtype):
    """lam_l = max(H_l, W_l) * (ulp of the arithmetic the bilinear weights are computed in)."""
    sh = np.asarray(torch.as_tensor(shapes).reshape(-1, 2).tolist(), dtype=np.float64)
    return sh.max(1) * LAM_ULP[dtype]


def term_sums(x, bilinear=True, level_scale=None, max_elems=1 << 22):
    """fp64, vectorised: for each output of the op, the sum over its terms of |term| -- with the bilinear weights
    (``bilinear=True``; out / grad_value / grad_attn then equal the oracle on |inputs|) or with every weight replaced by
    1 (A'), each level's terms multiplied by ``level_scale[l]``.  grad_loc's sum always has unit weights:
    |attn| * extent * sum_c |g_c| * sum_corners |v_c|.  Edge semantics are the kernel's (oracle/msda_ref_body.inc):
    strict range test on loc * extent - 0.5, corners outside the map skipped, non-finite locations contribute nothing.
    -> numpy (out [B, Nq, H*D], grad_value [B, S, H, D], grad_loc [B, Nq, H, L, P, 2], grad_attn [B, Nq, H, L, P])."""
    value = torch.as_tensor(x["value"]).double()
    loc, attn = torch.as_tensor(x["loc"]).double(), torch.as_tensor(x["attn"]).double()
    B, S, H, D = value.shape
    Nq, L, P = loc.shape[1], loc.shape[3], loc.shape[4]
    shapes = torch.as_tensor(x["shapes"]).reshape(-1, 2).tolist()
    start = torch.as_tensor(x["start"]).reshape(-1).tolist()
    aa = attn.abs()
    av = torch.cat((value.abs().reshape(B * S * H, D), value.new_zeros(1, D)))       # row B*S*H: corners off the map
    ag = torch.as_tensor(x["grad"]).double().reshape(B, Nq, H, D).abs()
    out = torch.zeros(B, Nq, H, D, dtype=torch.float64)
    gv_rows, gv_cols, gv_vals = [], [], []          # grad_value = (pixel row x sample's (b, q, h) weights) @ |grad|
    gl = torch.zeros(B, Nq, H, L, P, 2, dtype=torch.float64)
    ga = torch.zeros(B, Nq, H, L, P, dtype=torch.float64)
    bi = torch.arange(B).view(B, 1, 1, 1)
    hi = torch.arange(H).view(1, 1, H, 1)
    step = max(1, max_elems // max(1, B * H * P * D))
    for q0 in range(0, Nq, step):
        q1 = min(Nq, q0 + step)
        g = ag[:, q0:q1, :, None, :]                                        # [B, n, 1 -> H, 1 -> P, D]
        for l, ((Hl, Wl), s0) in enumerate(zip(shapes, start)):
            scale = 1.0 if level_scale is None else float(level_scale[l])
            px = loc[:, q0:q1, :, l, :, 0] * Wl - 0.5                       # [B, n, H, P]
            py = loc[:, q0:q1, :, l, :, 1] * Hl - 0.5
            inside = (py > -1) & (px > -1) & (py < Hl) & (px < Wl)
            px, py = torch.where(inside, px, 0.0), torch.where(inside, py, 0.0)
            x0, y0 = torch.floor(px), torch.floor(py)
            fx, fy = px - x0, py - y0
            a = aa[:, q0:q1, :, l] * scale
            vw = v1 = None                                                  # sum_corners w |v|, sum_corners |v|
            for dy in (0, 1):
                for dx in (0, 1):
                    yi, xi = y0 + dy, x0 + dx
                    ok = inside & (yi >= 0) & (yi <= Hl - 1) & (xi >= 0) & (xi <= Wl - 1)
                    row = ((bi * S + (s0 + yi * Wl + xi).long()) * H + hi)
                    row = torch.where(ok, row, B * S * H).reshape(-1)
                    rows = av.index_select(0, row).view(*ok.shape, D)
                    v1 = rows if v1 is None else v1 + rows
                    w = a * ok
                    if bilinear:
                        bw = (fy if dy else 1 - fy) * (fx if dx else 1 - fx) * ok
                        vw = bw[..., None] * rows if vw is None else vw + bw[..., None] * rows
                        w = w * bw
                    gv_rows.append(row)
                    gv_cols.append(((bi * Nq + q0 + torch.arange(q1 - q0).view(1, -1, 1, 1)) * H + hi).expand_as(ok).reshape(-1))
                    gv_vals.append(w.reshape(-1))
            vw = vw if bilinear else v1
            out[:, q0:q1] += (a[..., None] * vw).sum(3)
            ga[:, q0:q1, :, l] = (g * vw).sum(-1) * scale
            gsum = (g * v1).sum(-1) * a
            gl[:, q0:q1, :, l, :, 0] = gsum * Wl
            gl[:, q0:q1, :, l, :, 1] = gsum * Hl
    gv = torch.zeros(B * S * H + 1, D, dtype=torch.float64)
    if gv_rows:
        m = torch.sparse_coo_tensor(torch.stack((torch.cat(gv_rows), torch.cat(gv_cols))), torch.cat(gv_vals),
                                    (B * S * H + 1, B * Nq * H))
        gv = torch.sparse.mm(m, ag.reshape(B * Nq * H, D))
    return (out.reshape(B, Nq, H * D).numpy(), gv[:-1].reshape(B, S, H, D).numpy(), gl.numpy(), ga.numpy())


def error_bounds(x, dtype, gamma=None):
    """-> {output: bound array} (the right-hand side above, in the oracle's shapes) for inputs ``x`` (the dict of
    make_inputs: fp64 tensors holding storage-rounded numbers) and the storage type ``dtype``."""
    from oracle import msda_oracle
    gamma = GAMMA[dtype] if gamma is None else gamma
    assert gamma <= GAMMA_CEILING[dtype], (gamma, dtype)     # a route's own gamma stays under the ceiling
    u = STORAGE_U[dtype]
    v, sh, st, loc, at, gr = (x[k] for k in ("value", "shapes", "start", "loc", "attn", "grad"))
    a_out = msda_oracle.forward(v.abs(), sh, st, loc, at.abs())
    a_gv, _, a_ga = msda_oracle.backward(v.abs(), sh, st, loc, at.abs(), gr.abs())
    p_out, p_gv, p_gl, p_ga = term_sums(x, bilinear=False, level_scale=level_lams(sh, dtype))
    lams = level_lams(sh, dtype)
    # (unit weights: A and A' coincide; a (0, 0) level has lam 0 and grad_loc terms of 0 -- its A is 0, not 0 / 0)
    a_gl = p_gl / np.where(lams > 0, lams, 1.0)[None, None, None, :, None, None]
    ref = dict(zip(OUTPUTS, _oracle(x)))
    A = dict(out=(a_out, p_out), grad_value=(a_gv, p_gv), grad_loc=(a_gl, p_gl), grad_attn=(a_ga, p_ga))
    bounds = {n: u * np.abs(ref[n]) + STORAGE_T[dtype] * (A[n][0] > 0) + gamma * A[n][0] + A[n][1] for n in OUTPUTS}
    if dtype == torch.float16:
        ones = dict(x, attn=(torch.as_tensor(x["attn"]) != 0).double())        # (a zero weight makes no record)
        w_out, w_gv, _, w_ga = term_sums(ones, bilinear=False)
        for n, w in (("out", w_out), ("grad_value", w_gv), ("grad_attn", w_ga)):
            bounds[n] = bounds[n] + HALF_WEIGHT_FLOOR * w
    return bounds, ref


def _oracle(x):
    from oracle import msda_oracle
    out = msda_oracle.forward(x["value"], x["shapes"], x["start"], x["loc"], x["attn"])
    return (out,) + tuple(msda_oracle.backward(x["value"], x["shapes"], x["start"], x["loc"], x["attn"], x["grad"]))


def near_crossing(x):
    """[B, Nq, H, L, P, 2] bool: samples within NEAR_CROSSING of a pixel crossing (both coordinates flagged)."""
    sh = np.asarray(torch.as_tensor(x["shapes"]).reshape(-1, 2).tolist(), dtype=np.float64)
    pix = np.asarray(x["loc"], dtype=np.float64) * sh[None, None, None, :, None, ::-1] - 0.5
    with np.errstate(invalid="ignore"):
        near = (np.abs(pix - np.round(pix)) < NEAR_CROSSING).any(-1, keepdims=True)
    return np.broadcast_to(near, pix.shape)


def _where(name, idx, x):
    """Coordinates of a flat index into output ``name``, in the op's terms."""
    B, S, H, D = x["value"].shape
    Nq, L, P = x["loc"].shape[1], x["loc"].shape[3], x["loc"].shape[4]
    if name == "out":
        b, q, h, c = np.unravel_index(idx, (B, Nq, H, D))
        return f"b={b} q={q} h={h} c={c}"
    if name == "grad_value":
        b, s, h, c = np.unravel_index(idx, (B, S, H, D))
        shapes = torch.as_tensor(x["shapes"]).reshape(-1, 2).tolist()
        for l, ((Hl, Wl), s0) in enumerate(zip(shapes, torch.as_tensor(x["start"]).tolist())):
            if s0 <= s < s0 + Hl * Wl:
                return f"b={b} pixel={s} (level {l}, y={(s - s0) // Wl} x={(s - s0) % Wl}) h={h} c={c}"
        return f"b={b} pixel={s} (no level) h={h} c={c}"
    if name == "grad_loc":
        b, q, h, l, p, k = np.unravel_index(idx, (B, Nq, H, L, P, 2))
        return f"b={b} q={q} h={h} level={l} p={p} {'xy'[k]}"
    b, q, h, l, p = np.unravel_index(idx, (B, Nq, H, L, P))
    return f"b={b} q={q} h={h} level={l} p={p}"


def bound_ratios(got, x, dtype, outputs=OUTPUTS, want=None, gamma=None, bounds=None):
    """Worst |got - ref| / bound per output, with where it is: {name: (ratio, "coordinates", error, bound)}.
    ``got`` is a sequence in OUTPUTS order (entries of outputs not listed may be None).  ``want`` replaces the
    oracle's reference (tests that zero entries on purpose); ``bounds`` reuses error_bounds(x, dtype, gamma)[0].
    Non-finite entries: finiteness must match (ratio inf otherwise) and only finite ones are compared; an element whose
    bound is 0 must be exactly right (ratio inf otherwise); grad_loc leaves out samples near a pixel crossing."""
    if bounds is None:
        bounds, ref = error_bounds(x, dtype, gamma)
    else:
        ref = dict(zip(OUTPUTS, _oracle(x)))
    if want is not None:
        ref = dict(zip(OUTPUTS, want))
    res = {}
    for name in outputs:
        i = OUTPUTS.index(name)
        r = np.asarray(ref[name], dtype=np.float64)
        g = np.asarray(got[i], dtype=np.float64).reshape(r.shape)
        bnd = np.broadcast_to(bounds[name], r.shape)
        fin = np.isfinite(r)
        if not np.array_equal(np.isfinite(g), fin):
            k = int(np.flatnonzero(np.isfinite(g) != fin)[0])
            res[name] = (float("inf"), _where(name, k, x) + " (finiteness differs)", float(g.flat[k]), float(r.flat[k]))
            continue
        use = fin & np.isfinite(bnd)
        if name == "grad_loc":
            use &= ~near_crossing(x)
        with np.errstate(invalid="ignore", divide="ignore"):
            err = np.where(use, np.abs(g - r), 0.0)
            ratio = np.where(bnd > 0, err / np.where(bnd > 0, bnd, 1.0), np.where(err > 0, np.inf, 0.0))
        k = int(np.argmax(ratio)) if ratio.size else 0
        res[name] = ((float(ratio.flat[k]), _where(name, k, x), float(err.flat[k]), float(bnd.flat[k]))
                     if ratio.size else (0.0, "-", 0.0, 0.0))
    return res


def assert_within_bounds(got, x, dtype, what="", outputs=OUTPUTS, want=None, gamma=None, report=None):
    """Assert bound_ratios(...) <= 1 for every listed output; ``report`` (a dict) collects the worst ratios."""
    res = bound_ratios(got, x, dtype, outputs, want=want, gamma=gamma)
    if report is not None:
        for n, r in res.items():
            report[n] = max(report.get(n, 0.0), r[0])
    bad = {n: r for n, r in res.items() if not r[0] <= 1.0}
    assert not bad, f"{what}: per-element bound broken: " + "; ".join(
        f"{n} {r[0]:.3g} x the bound at {r[1]} (err {r[2]:.3e}, bound {r[3]:.3e})" for n, r in bad.items())
    return res


# ---------------------------------------------------------------------------------------------------------------------
# Problems too large for the oracle as a whole (tests/test_large_slabs*.py): the op's heads are independent -- output
# head h reads value, loc, attn and grad at head h only -- so restricting the inputs and every output to a set of heads is
# the same op on a smaller problem, and the oracle and the bound above serve it unchanged.
# ---------------------------------------------------------------------------------------------------------------------
def head_subset(x, heads):
    """-> the input dict of make_inputs reduced to ``heads`` (in that order): value [B, S, n, D], loc [B, Nq, n, L, P, 2],
    attn [B, Nq, n, L, P], grad [B, Nq, n * D]; the level table and every other key as they are.  Tensors stay on their
    device and keep their type (the caller rounds / moves them)."""
    value, loc, attn = (torch.as_tensor(x[k]) for k in ("value", "loc", "attn"))
    B, S, H, D = value.shape
    Nq = loc.shape[1]
    pick = lambda t: t.index_select(2, torch.as_tensor(list(heads), dtype=torch.long, device=t.device))
    grad = pick(torch.as_tensor(x["grad"]).reshape(B, Nq, H, D))
    return dict(x, value=pick(value), loc=pick(loc), attn=pick(attn), grad=grad.reshape(B, Nq, -1))


def head_subset_outputs(outs, heads, H):
    """The op's outputs in OUTPUTS order (entries may be None) at ``heads``: out [B, Nq, n * D], grad_value
    [B, S, n, D], grad_loc [B, Nq, n, L, P, 2], grad_attn [B, Nq, n, L, P]."""
    pick = lambda t: t.index_select(2, torch.as_tensor(list(heads), dtype=torch.long, device=t.device))
    res = []
    for name, t in zip(OUTPUTS, outs):
        if t is None:
            res.append(None)
        elif name == "out":
            B, Nq = t.shape[:2]
            res.append(pick(t.reshape(B, Nq, H, -1)).reshape(B, Nq, -1))
        else:
            res.append(pick(t))
    return res


def worst_ratio(got, ref, bound, skip=None):
    """bound_ratios' rule for ONE output on torch tensors, on whatever device they live (an output of 10^8 elements is
    compared where it was computed): ``ref`` and ``bound`` fp64 of the output's shape, ``skip`` bool (grad_loc's samples
    near a pixel crossing) or None.  -> (ratio, flat index, error, bound); finiteness that differs, or an error where the
    bound is 0, gives inf."""
    ref, bound = ref.double(), bound.double().expand(ref.shape)
    g = got.double().reshape(ref.shape)
    if g.numel() == 0:
        return 0.0, 0, 0.0, 0.0
    fin = torch.isfinite(ref)
    odd = torch.isfinite(g) != fin
    if bool(odd.any()):
        k = int(odd.reshape(-1).nonzero()[0])
        return float("inf"), k, float(g.reshape(-1)[k]), float(ref.reshape(-1)[k])
    use = fin & torch.isfinite(bound)
    if skip is not None:
        use &= ~skip
    zero, inf = torch.zeros((), dtype=torch.float64, device=g.device), torch.full((), float("inf"), dtype=torch.float64, device=g.device)
    err = torch.where(use, (g - ref).abs(), zero)
    pos = bound > 0
    ratio = torch.where(pos, err / torch.where(pos, bound, zero + 1.0), torch.where(err > 0, inf, zero))
    k = int(ratio.reshape(-1).argmax())
    return float(ratio.reshape(-1)[k]), k, float(err.reshape(-1)[k]), float(bound.reshape(-1)[k])
