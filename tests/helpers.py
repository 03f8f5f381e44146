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


# ---------------------------------------------------------------------------------------------------------------------
# Placement: operands at the least alignment an entry point accepts, and outputs between guard bands.
#
# Every tensor torch's allocator hands out is 512-byte aligned and has slack behind it, so a branch a kernel takes on a
# pointer's alignment never runs, and a store a few elements outside an output lands in memory nobody looks at.
# ``placed`` puts a tensor at a chosen byte offset from a 256-byte boundary, inside a buffer the test owns, between two
# guard bands; ``guarded_allocations`` does the same to what the code under test allocates.
#
# What the guards catch: a store within GUARD_BYTES before or behind a placed tensor (the band is compared byte for
# byte), and -- with 0xFF input guards, NaN in every floating type here and -1 in the integer tables -- a read outside
# an input that reaches a result (the result then differs from the run on ordinary allocations).  What they do not
# catch: a store further out than GUARD_BYTES (64 KiB is a condition of the check, not a measurement of how far a stray
# store can go), a stray store that writes the guard's own byte value, and a stray read whose value is multiplied away
# or never used.
# ---------------------------------------------------------------------------------------------------------------------
GUARD_BYTES = 64 * 1024
PLACE_ALIGN = 256
_raw_empty = torch.empty               # (guarded_allocations replaces torch.empty: the buffers themselves come from this)
INPUT_GUARD, OUTPUT_GUARD = 0xFF, 0xA5


class Placed:
    """A tensor inside a guarded byte buffer: ``t`` the tensor, ``buf`` the whole buffer (uint8), ``lo`` / ``hi`` the
    payload's byte range in it, ``fill`` the guards' byte, ``name`` what messages call it, ``before`` a copy of the
    payload's bytes as they were put in (inputs) or None."""
    __slots__ = ("t", "buf", "lo", "hi", "fill", "name", "before")

    def __init__(self, t, buf, lo, hi, fill, name):
        self.t, self.buf, self.lo, self.hi, self.fill, self.name, self.before = t, buf, lo, hi, fill, name, None

    def payload(self):
        return self.buf[self.lo:self.hi]


def _place(shape, strides, dtype, device, lead, guard_fill, name):
    """A guarded buffer and a tensor of ``shape`` / ``strides`` (None: contiguous) in it whose first element lies ``lead``
    bytes past a PLACE_ALIGN boundary.  The payload is left as the guard byte."""
    es = _raw_empty((), dtype=dtype).element_size()
    assert lead >= 0 and lead % es == 0, f"{name}: a lead of {lead} bytes is no multiple of the {es}-byte element"
    shape = tuple(int(s) for s in shape)
    numel = int(np.prod(shape, dtype=np.int64)) if shape else 1
    if strides is None:
        span = numel
    else:
        span = 1 + sum((n - 1) * s for n, s in zip(shape, strides)) if numel else 0
        assert span == numel, f"{name}: strides {strides} of shape {shape} are not dense"
    nbytes = span * es
    buf = _raw_empty(2 * GUARD_BYTES + PLACE_ALIGN + lead + nbytes, dtype=torch.uint8, device=device)
    buf.fill_(guard_fill)
    lo = GUARD_BYTES + (-(buf.data_ptr() + GUARD_BYTES)) % PLACE_ALIGN + lead
    flat = buf[lo:lo + nbytes].view(dtype)
    t = flat.view(shape) if strides is None else flat.as_strided(shape, strides)
    assert numel == 0 or (t.data_ptr() - lead) % PLACE_ALIGN == 0
    return Placed(t, buf, lo, lo + nbytes, guard_fill, name)


def placed(t, lead=0, guard_fill=INPUT_GUARD, device=None, name="tensor"):
    """-> Placed: a contiguous copy of ``t`` (on ``device``, default ``t``'s) that starts ``lead`` bytes past a 256-byte
    boundary, with at least GUARD_BYTES of ``guard_fill`` bytes on either side (0xFF for inputs, 0xA5 for outputs).  The
    copy is ``.t``; its bytes as put in are kept for ``assert_payload_unchanged``.  A store further than GUARD_BYTES from
    the tensor is not seen (above)."""
    src = t.detach().contiguous()
    h = _place(src.shape, None, src.dtype, torch.device(device) if device is not None else src.device, lead, guard_fill, name)
    h.t.copy_(src)
    h.before = h.payload().clone()
    return h


def _first_bad(band, fill):
    bad = (band != fill).nonzero()
    return None if bad.numel() == 0 else (int(bad[0]), int(bad[-1]), int(bad.numel()))


def guard_damage(h):
    """None, or a sentence on where the guards of ``h`` no longer hold their byte."""
    below = _first_bad(h.buf[:h.lo], h.fill)
    above = _first_bad(h.buf[h.hi:], h.fill)
    msgs = []
    if below is not None:
        msgs.append(f"{below[2]} byte(s) changed BEFORE the start, the nearest {h.lo - below[1]} byte(s) before it")
    if above is not None:
        msgs.append(f"{above[2]} byte(s) changed PAST the end, the nearest {above[0]} byte(s) past it")
    return "; ".join(msgs) or None


def guards_intact(h):
    """Both guard bands of ``h`` (a Placed) still hold their byte, compared byte for byte."""
    return guard_damage(h) is None


def assert_guards_intact(*handles):
    bad = [f"{h.name}: {d}" for h in handles for d in [guard_damage(h)] if d]
    assert not bad, "written outside a tensor: " + " | ".join(bad)


def assert_payload_unchanged(*handles):
    """Every placed INPUT holds, bit for bit, what was put in."""
    for h in handles:
        diff = (h.payload() != h.before).nonzero()
        es = h.t.element_size()
        assert diff.numel() == 0, (f"input {h.name} {tuple(h.t.shape)} was modified: {int(diff.numel())} byte(s), the first "
                                   f"in element {int(diff[0]) // es}")


def _bytes(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8) if t.numel() else t.detach().reshape(-1).view(torch.uint8)


def assert_bit_equal(got, want, name):
    """Same shape, type and bytes (NaN payloads and signed zeros included)."""
    assert got.shape == want.shape and got.dtype == want.dtype, f"{name}: {tuple(got.shape)} {got.dtype} vs {tuple(want.shape)} {want.dtype}"
    diff = (_bytes(got) != _bytes(want).to(got.device)).nonzero()
    if diff.numel():
        k = int(diff[0]) // got.element_size()
        g, w = got.detach().contiguous().reshape(-1)[k], want.detach().contiguous().reshape(-1)[k]
        raise AssertionError(f"{name}: {len(set((diff.reshape(-1) // got.element_size()).tolist()))} element(s) differ, the first "
                             f"at flat index {k}: {g.item()!r} vs {w.item()!r}")


def poison_left(t):
    """How many elements of ``t`` still hold ``poison``'s pattern (NaN counts for the floating types: use on results that
    are finite)."""
    if t.numel() == 0:
        return 0
    t = t.detach()
    if t.is_floating_point():
        if t.element_size() == 1:
            return int((t.contiguous().view(torch.uint8) == 0xFF).sum())
        return int(torch.isnan(t).sum())
    ref = _raw_empty((), dtype=t.dtype)
    _fill_poison(ref)
    return int((t == ref.to(t.device)).sum())


def assert_no_poison(t, name):
    n = poison_left(t)
    assert n == 0, (f"{name} {tuple(t.shape)}: {n} element(s) hold the allocation's poison: nobody wrote them -- or, of a "
                    f"floating type, a NaN read outside an input's extent reached them")


class GuardedAllocations:
    """What ``guarded_allocations`` recorded: ``records`` (a Placed per allocation it placed, named by the allocating
    line), ``passed_through`` (a description per allocation on the guarded device it could not place)."""

    def __init__(self):
        self.records, self.passed_through = [], []

    @property
    def pass_through_count(self):
        return len(self.passed_through)

    def assert_all_intact(self):
        assert_guards_intact(*self.records)


def _dense(shape, strides):
    """The strides are a permutation of a contiguous layout: every element of the span is owned once."""
    want = 1
    for n, s in sorted(((n, s) for n, s in zip(shape, strides) if n != 1), key=lambda p: p[1]):
        if s != want:
            return False
        want *= n
    return True


def _caller(depth=2):
    import sys
    f = sys._getframe(depth)
    return f"{os.path.basename(f.f_code.co_filename)}:{f.f_lineno}"


def guarded_allocations(monkeypatch, device="cuda"):
    """For the rest of a test: torch.empty / torch.empty_like / torch.zeros / Tensor.new_zeros on a ``device``-type device
    hand out tensors placed (lead 0) between OUTPUT_GUARD bands of GUARD_BYTES each -- the payload poisoned as ``poison``
    does, zero for the two zeros forms -- and every one is recorded.  -> GuardedAllocations.  Allocations on other devices
    (meta, and the CPU unless ``device="cpu"``), pinned ones and empty ones pass through untouched; one on the guarded
    device whose layout is not dense (no such request exists in the package today) passes through and is counted.  A
    dense non-default ``memory_format`` is reproduced with ``as_strided`` inside the buffer.  A store further than
    GUARD_BYTES from its tensor is not seen."""
    rec = GuardedAllocations()
    kind = torch.device(device).type
    orig = dict(empty=torch.empty, empty_like=torch.empty_like, zeros=torch.zeros, new_zeros=torch.Tensor.new_zeros)

    def guard(r, zero, site):
        if not isinstance(r, torch.Tensor) or r.device.type != kind or r.numel() == 0 or r.layout != torch.strided:
            return r
        if kind == "cpu" and r.is_pinned():
            return r
        what = f"{tuple(r.shape)} {str(r.dtype)[6:]} allocated at {site}"
        dense = r.is_contiguous() or _dense(r.shape, r.stride())
        if not dense or r.is_complex() or r.is_quantized:
            rec.passed_through.append(what)
            return r
        with torch.no_grad():
            h = _place(r.shape, None if r.is_contiguous() else r.stride(), r.dtype, r.device, 0, OUTPUT_GUARD, what)
            h.t.zero_() if zero else _fill_poison(h.t)
        if r.requires_grad:
            h.t.requires_grad_(True)
        rec.records.append(h)
        return h.t

    def wrap(name, zero):
        fn = orig[name]

        def patched(*a, **k):
            if k.get("out") is not None:
                return fn(*a, **k)
            return guard(fn(*a, **k), zero, _caller())
        patched.__name__ = name
        return patched

    monkeypatch.setattr(torch, "empty", wrap("empty", False))
    monkeypatch.setattr(torch, "empty_like", wrap("empty_like", False))
    monkeypatch.setattr(torch, "zeros", wrap("zeros", True))
    monkeypatch.setattr(torch.Tensor, "new_zeros", wrap("new_zeros", True))
    return rec


def run_placed(monkeypatch, fn, inputs, leads=None, device="cuda", bit_equal=True, allowed_pass_through=(), writes=()):
    """The whole yardstick around one call.  ``fn(**tensors)`` -> a tensor or a sequence of tensors (None entries allowed),
    allocating its outputs and workspaces itself; ``inputs``: {name: tensor}.  Runs ``fn`` on ordinary allocations, then
    on inputs placed (``leads[name]`` bytes past a 256-byte boundary, default 0) between 0xFF guards under
    ``guarded_allocations``, and asserts: no guard of an input or of a recorded allocation changed; every input holds what
    was put in (but those named in ``writes``: tensors the call updates in place, a cache); no returned element is left poisoned; nothing passed through unplaced but ``allowed_pass_through``
    (descriptions, matched as substrings); and, with ``bit_equal``, every returned tensor equals the ordinary run's bit for
    bit -- a read outside an input would meet NaN / -1.  -> (placed run's outputs, ordinary run's outputs, recorder)."""
    sync = torch.cuda.synchronize if torch.device(device).type == "cuda" else (lambda: None)
    as_list = lambda r: [r] if isinstance(r, torch.Tensor) else list(r)
    plain = as_list(fn(**{k: v.to(device).clone() for k, v in inputs.items()}))
    sync()
    handles = {k: placed(v, (leads or {}).get(k, 0), INPUT_GUARD, device, name=k) for k, v in inputs.items()}
    with monkeypatch.context() as m:
        rec = guarded_allocations(m, device)
        got = as_list(fn(**{k: h.t for k, h in handles.items()}))
        sync()
    assert_guards_intact(*handles.values())
    rec.assert_all_intact()
    assert_payload_unchanged(*[h for k, h in handles.items() if k not in writes])
    stray = [w for w in rec.passed_through if not any(a in w for a in allowed_pass_through)]
    assert not stray, f"allocations that could not be placed between guards: {stray}"
    assert len(got) == len(plain)
    for i, (g, w) in enumerate(zip(got, plain)):
        if g is None or w is None:
            assert g is None and w is None, f"output {i}: one run returned None"
            continue
        assert_no_poison(g, f"output {i}")
        if bit_equal:
            assert_bit_equal(g, w, f"output {i} (placed inputs and guarded allocations vs ordinary ones)")
    return got, plain, rec


# ---------------------------------------------------------------------------------------------------------------------
# The op's inputs of tests/test_placement_gpu.py, shared with tests/test_placement.py (which checks on the CPU what share
# of their samples ``near_crossing`` leaves out of the grad_loc comparison).
# ---------------------------------------------------------------------------------------------------------------------
# the smallest shape with a ragged query tile (33 queries) and two levels, neither a multiple of the 4x4 block
OP_SHAPE = dict(B=1, H=2, Nq=33, P=4, shapes=[(5, 7), (2, 3)])
OP_SEED = 61
OP_DTYPES = (torch.bfloat16, torch.float16, torch.float32)
# head widths: 32 (every route of the backward), 128 (what the LDS-resident forwards take)
OP_WIDTHS = (32, 128)
MAX_LEFT_OUT = 0.01          # share of grad_loc's samples ``near_crossing`` may leave out, per case


def op_inputs(dtype, D=32, seed=OP_SEED, loc_range=(-0.1, 1.1)):
    s = OP_SHAPE
    return make_inputs(s["B"], s["H"], D, s["Nq"], s["P"], s["shapes"], seed=seed, loc_range=loc_range, dtype=dtype)


def hot_inputs(dtype, D=64):
    """Every location of a slice within one cell of each level (the "point" distribution of tests/fuzz_op.py: loc in
    [0.45, 0.47]).  On the 8 x 8 level that cell's footprint is pixels 3 and 4 in both directions, so it straddles the four 4x4
    blocks that meet there: each of them gets all 6000 samples of a slice -- more than a work item's records (768 at D = 64:
    csrc/msda_bwd_block.h ``tile_chunk``), so the blocks' lists are cut into chunks -- the backward workspace's data-dependent
    writers."""
    x = make_inputs(1, 2, D, 1500, 4, [(8, 8), (4, 4)], seed=5, dtype=dtype)
    x["loc"] = (x["loc"] * 0.02 + 0.45).to(dtype).double()
    return x


def pair_inputs(dtype, D=32):
    """One 4 x 8 level = one pair of whole 4x4 blocks (the smallest case of tests/test_tile_pair_gpu.py), the locations moved
    onto a grid of 64ths plus 1/256: on 16-bit grids a uniform draw puts 3.6 % of the samples ON a pixel crossing of a level
    whose extents are powers of two; here none is closer to one than 1/32 of a pixel."""
    x = make_inputs(1, 2, D, 24, 4, [(4, 8)], seed=41, dtype=dtype)
    x["loc"] = (torch.round(x["loc"] * 64) / 64 + 1.0 / 256).to(dtype).double()
    return x


KINDS = {"ragged": op_inputs, "hot": hot_inputs, "pair": pair_inputs}
ODD_D = 6            # rows of 12 bytes (16-bit storage) and 24 (fp32): the C contract's ``row_align`` is the element size


def op_cases():
    """(id, inputs) of every input set the placement tests hold grad_loc on."""
    for dtype in OP_DTYPES:
        for D in OP_WIDTHS + (ODD_D,):
            yield f"{str(dtype)[6:]}-D{D}", op_inputs(dtype, D)
        yield f"{str(dtype)[6:]}-hot", hot_inputs(dtype)
        yield f"{str(dtype)[6:]}-pair", pair_inputs(dtype)
