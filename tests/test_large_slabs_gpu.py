"""The op at (batch, head) slabs on both sides of 2 GiB, and past 4 GiB: the flat-address branches of the kernels
(BUF = false), the refusals of the kernels that only have 32-bit row offsets, and the 64-bit batch offsets.

A buffer descriptor spans kMaxSlabBytes = 2^31 - 1 bytes (csrc/msda_device.h).  The value slab of a sample is
S * H * D * es bytes, the grad_out slab Nq * H * D * es; here H * D * es = 65536 in every variant, so the limits fall
on whole rows:

    case      level table / Nq                         what it crosses
    V-under   [(181,181),(2,3)]  S = 32767, B = 2      value slab 2^31 - 65536: still the buffer path; batch 1 starts past
                                                       2^31 bytes, the tensor has > 2^31 elements (fp32: > 2^32 bytes)
    V-over    [(181,181),(1,7)]  S = 32768             value slab = 2^31: the first size on the flat path
    V-far     [(256,256),(2,2)]  S = 65540             value slab > 2^32: 32-bit byte products wrap, one level is 4 GiB
    G-under / G-over / G-far   [(12,12),(5,7)], Nq = 32767 / 32770 / 65540: the same three for the grad_out slab
    VG-over   S = 32768 and Nq = 32770                 both at once (encoder self-attention: Nq = S)

Reference.  The op's heads are independent, so its outputs at 8 heads (0, H - 1 and six seeded others) are the op on the
problem reduced to those heads (helpers.head_subset; tests/test_large_slabs.py): the fp64 oracle and the per-element
bound of helpers.py, constants unchanged, applied with helpers.worst_ratio where the outputs live.  Inputs are made on the
device from a seeded generator in the storage type; only the 8 heads travel to the host.  Every allocation of the op is
poisoned.  In the G cases the first level's samples of all queries stay in columns >= 4 of the 12 x 12 map, except those
of queries 32766 .. 32769 (those that exist), each of which sits alone on pixels of its own in columns 1 .. 2: a query
whose grad_out row is dropped leaves exact zeros where only it contributes.

Whole-tensor nets, on the device over all heads (they catch gross misaddressing outside the 8 heads, nothing finer): no
non-finite output element; every output within TOL[dtype] * max|ref| (the bar of tests/test_op_gpu.py) of the same op
run on contiguous chunks of 32 heads -- small-slab calls through routes the rest of the suite holds to the oracle --; and
grad_value's (b, pixel, head) rows all-zero exactly where the chunked runs' are: a dropped row leaves a zero row, a stray one
a row where nothing belongs.  (Per ROW, not per element: whether a floating-point sum that cancels comes out as 0 or as a
rounding residue depends on the order and the precision of the products, which differ between routes, and with 8-bit
significands the terms of an element do cancel exactly now and then: profiles/large_slabs.md, section 3.  A row of D such
sums cancelling together does not happen.)

Routes.  Every forward kernel of FWD_ALGOS and every backward route of BWD_ROUTES (tests/test_level_geometry_gpu.py; what
ran is read off the entry points the shim called, as there).  A named forward kernel, or the named LDS-levels taps kernel,
that cannot take a slab over the limit hands the call to the row gather: its result must be torch.equal to "gather"'s,
and MSDA._event_log must show that launch alone ("msda_fwd_gather").  A backward route refused for the size must give the
fallback's numbers, not an error.  Refusals for the KIND of the arguments still raise (fp32 storage has no matrix-core
forward; D = 32 no query-wave kernel) and are recorded as such.  At 16-bit storage the V cases run P = 4: the sorted
route's scan and the MMFS sampler take whole 16-byte vectors of locations; everything else runs L = 2, P = 2.

Memory: each test states its peak, asks torch.cuda.mem_get_info() first, frees what it made.  None needs over 24 GiB
(V-far through the float-atomic route, whose fp32 image is twice the bank, 4 + 4 + 8 GiB + workspace, stays under it --
so nothing of V-far is left out)."""
import contextlib
import random
import time

import numpy as np
import pytest
import torch

import helpers
from helpers import OUTPUTS, error_bounds, head_subset, head_subset_outputs, level_tables, near_crossing, worst_ratio
from test_level_geometry_gpu import BWD_ROUTES, FWD_ALGOS, entry_calls, evidence, knobs
from test_op_gpu import TOL

pytestmark = pytest.mark.gpu
DEV = "cuda"
GIB = 1 << 30
LIMIT = 0x7fffffff                      # kMaxSlabBytes
ROW_BYTES = 65536
CHUNK = 32                              # heads per small-slab run of the nets

VARIANTS = {                            # storage type, H, D: H * D * es = 65536
    "bf16": (torch.bfloat16, 256, 128),
    "fp32": (torch.float32, 128, 128),
    "bf16-H1024": (torch.bfloat16, 1024, 32),
}
V_TABLES = {"under": [(181, 181), (2, 3)], "over": [(181, 181), (1, 7)], "far": [(256, 256), (2, 2)]}
G_TABLE = [(12, 12), (5, 7)]
G_NQ = {"under": 32767, "over": 32770, "far": 65540}
LONE = (32766, 32767, 32768, 32769)     # G cases: queries around byte offset 0x80000000 of the grad_out slab
#          shapes, Nq, B, GiB of free device memory asked for: the measured peak (torch.cuda.max_memory_allocated(), MI355X,
#          profiles/large_slabs.md) plus ~2 GiB, and never over the 24 GiB that every test must fit in
CASES = {
    "V-under": (V_TABLES["under"], 48, 2, 21),     # 19.0: bank 4 + grad_value 4 + fp32 image (atomic, device-checked) 8 + the rest
    "V-over": (V_TABLES["over"], 48, 1, 12),       # 9.5
    "V-far": (V_TABLES["far"], 48, 1, 21),         # 19.0 (fp32 18.0): bank 4 + grad_value 4 + fp32 image 8 + the rest
    "G-under": (G_TABLE, G_NQ["under"], 1, 14),    # 11.8: grad_out 2 + out 2 x 2 (two kernels' results compared) + workspace
    "G-over": (G_TABLE, G_NQ["over"], 1, 14),      # 11.8
    "G-far": (G_TABLE, G_NQ["far"], 1, 24),        # 23.5 (fp32 22.6): the largest, under the 24 GiB every test must fit in
    "VG-over": (V_TABLES["over"], G_NQ["over"], 1, 17),   # 14.8
}
RUNS = [(c, v) for c in CASES for v in ("bf16", "fp32")] + [("VG-over", "bf16-H1024")]
# the third variant: one forward and one backward route
ONLY = {"bf16-H1024": (("gather",), ("value=pixel",))}


def slab_class(case):
    """(value slab over the limit, grad_out slab over the limit)"""
    shapes, Nq, _, _ = CASES[case]
    S = sum(h * w for h, w in shapes)
    return S * ROW_BYTES > LIMIT, Nq * ROW_BYTES > LIMIT


def points(case, dtype):
    return 4 if case.startswith("V-") and dtype != torch.float32 else 2


def need_memory(gib, what):
    free, _ = torch.cuda.mem_get_info()
    if free < gib * GIB:
        pytest.skip(f"{what}: needs {gib} GiB of device memory, {free / GIB:.1f} GiB free")


@contextlib.contextmanager
def released():
    try:
        yield
    finally:
        import gc
        gc.collect()
        torch.cuda.empty_cache()


@pytest.fixture
def poisoned(monkeypatch):
    helpers.poison_allocations(monkeypatch)
    yield


def selected_heads(H, seed):
    return [0] + sorted(random.Random(seed).sample(range(1, H - 1), 6)) + [H - 1]


def device_inputs(case, variant, seed):
    """The input dict of helpers.make_inputs, on the device, in the storage type (so already rounded through it)."""
    dtype, H, D = VARIANTS[variant]
    shapes, Nq, B, _ = CASES[case]
    P = points(case, dtype)
    g = torch.Generator(device=DEV).manual_seed(seed)
    sh, start = level_tables(shapes)
    S, L = int(sh.prod(1).sum()), sh.shape[0]
    value = torch.rand(B, S, H, D, generator=g, device=DEV, dtype=dtype)
    loc = torch.rand(B, Nq, H, L, P, 2, generator=g, device=DEV, dtype=torch.float32) * 1.3 - 0.15
    attn = torch.rand(B, Nq, H, L, P, generator=g, device=DEV, dtype=torch.float32) + 1e-5
    attn = attn / attn.sum((-1, -2), keepdim=True)
    if shapes == G_TABLE:
        loc[:, :, :, 0, :, 0] = loc[:, :, :, 0, :, 0] * (0.7 / 1.3) + 0.45 + 0.15 * (0.7 / 1.3)     # x in [0.45, 1.15): columns >= 4
        for i, q in enumerate(LONE):
            if q < Nq:      # pixel (3 i + 0.3, 1.3): rows 3 i, 3 i + 1, columns 1, 2 -- this query's alone
                loc[:, q, :, 0, :, 0] = 1.8 / 12
                loc[:, q, :, 0, :, 1] = (3 * i + 0.8) / 12
    loc, attn = loc.to(dtype), attn.to(dtype)
    loc[0, 1, 0, 0, 0, 0] = float("nan")              # a non-finite location: no contribution, zero gradients
    attn[0, 2, H - 1] = 0.0                           # zero weights: grad_value gets nothing, grad_attn is not zero
    grad = torch.randn(B, Nq, H * D, generator=g, device=DEV, dtype=dtype)
    return dict(value=value, shapes=sh, start=start, loc=loc, attn=attn, grad=grad)


class Reference:
    """Oracle and bound of the problem at the selected heads, uploaded: ref / bound [name] fp64 on the device."""

    def __init__(self, x, heads, dtype):
        self.heads, self.dtype = heads, dtype
        sub = head_subset(x, heads)
        self.x = {k: (v.double().cpu() if v.is_floating_point() else v.cpu()) for k, v in sub.items()}
        bounds, ref = error_bounds(self.x, dtype)
        self.ref = {n: torch.as_tensor(np.ascontiguousarray(ref[n])).to(DEV) for n in OUTPUTS}
        self.bound = {n: torch.as_tensor(np.array(np.broadcast_to(bounds[n], ref[n].shape))).to(DEV) for n in OUTPUTS}
        self.skip = torch.as_tensor(np.array(near_crossing(self.x))).to(DEV)
        self.worst = {}

    def fails(self, outs, H, what):
        """outs in OUTPUTS order (None: not computed) -> failure lines; the worst ratios are kept."""
        lines = []
        for name, t in zip(OUTPUTS, head_subset_outputs(outs, self.heads, H)):
            if t is None:
                continue
            r = worst_ratio(t, self.ref[name], self.bound[name], self.skip if name == "grad_loc" else None)
            self.worst[name] = max(self.worst.get(name, 0.0), r[0])
            if not r[0] <= 1.0:
                where = helpers._where(name, r[1], self.x)
                lines.append(f"{what}: {name} {r[0]:.3g} x the bound at {where} of heads {self.heads} (err {r[2]:.3e}, bound {r[3]:.3e})")
        return lines


def run_forward(MSDA, x, algo="auto"):
    """-> (out, launches logged) or the refusal's text"""
    dev = lambda t: t.to(DEV)
    log = []
    with knobs(MSDA, fwd=algo):
        MSDA._event_log = log
        try:
            out = MSDA.ms_deform_attn_forward(x["value"], dev(x["shapes"]), dev(x["start"]), x["loc"], x["attn"], 1)
            torch.cuda.synchronize()
        except RuntimeError as e:
            return str(e), [n for n, _, _ in log]
        finally:
            MSDA._event_log = None
    return out, [n for n, _, _ in log]


def run_backward(MSDA, x, cfg):
    """-> ([grad_value, grad_loc, grad_attn], what ran) or (the refusal's text, what ran)"""
    sh, st = x["shapes"].to(DEV), x["start"].to(DEV)             # (fresh tensors: unregistered unless registered here)
    if cfg["register"]:
        MSDA.register_level_tables(sh, st, x["value"].shape[1], host_shapes=x["shapes"], host_start=x["start"])
    B, Nq = x["loc"].shape[:2]
    with knobs(MSDA, **cfg), entry_calls(MSDA) as calls:
        try:
            grads = MSDA.ms_deform_attn_backward(x["value"], sh, st, x["loc"], x["attn"], x["grad"].reshape(B, Nq, -1), 1)
            torch.cuda.synchronize()
        except RuntimeError as e:
            return str(e), evidence(MSDA, calls)
    return list(grads), evidence(MSDA, calls)


def chunk_nets(MSDA, x, outs, dtype, what):
    """The whole-tensor nets of ``outs`` (OUTPUTS order, None: not computed) -> failure lines."""
    lines = []
    H = x["value"].shape[2]
    for name, t in zip(OUTPUTS, outs):
        if t is not None and not bool(torch.isfinite(t).all()):
            # (the one planted NaN location gives zeros, not NaN: nothing non-finite may come out)
            lines.append(f"{what}: {name} has non-finite elements")
    backward = any(t is not None for t in outs[1:])
    for h0 in range(0, H, CHUNK):
        hs = range(h0, min(H, h0 + CHUNK))
        sub = {k: (v.contiguous() if torch.is_tensor(v) and v.is_cuda else v) for k, v in head_subset(x, hs).items()}
        want = [None] * 4
        if outs[0] is not None:
            want[0] = run_forward(MSDA, sub)[0]
        if backward:
            grads = run_backward(MSDA, sub, dict(register=True))[0]
            assert isinstance(grads, list), f"{what}: the chunked run of heads {h0}.. was refused: {grads}"
            want[1:] = grads
        for name, got, ref in zip(OUTPUTS, head_subset_outputs(outs, hs, H), want):
            if got is None:
                continue
            assert torch.is_tensor(ref), f"{what}: the chunked run of heads {h0}.. was refused: {ref}"
            scale = float(ref.double().abs().max())
            err = float((got.double() - ref.double().reshape(got.shape)).abs().max())
            if not err <= TOL[dtype] * scale:
                lines.append(f"{what}: {name} heads {h0}..{hs[-1]}: {err:.3e} from the chunked run, bar {TOL[dtype]:.0e} * {scale:.3g}")
            if name == "grad_value":
                # per (b, pixel, head) row: see the module's docstring for why not per element
                live, want_live = (got != 0).any(-1), (ref.reshape(got.shape) != 0).any(-1)
                if not torch.equal(live, want_live):
                    odd = (live != want_live).nonzero()
                    shown = "; ".join(f"(b, pixel, head) = ({i[0]}, {i[1]}, {h0 + i[2]}): max |row| {float(got[tuple(i)].abs().max()):.3e} against "
                                      f"{float(ref.reshape(got.shape)[tuple(i)].abs().max()):.3e}" for i in odd[:4].tolist())
                    lines.append(f"{what}: grad_value heads {h0}..{hs[-1]}: {len(odd)} rows are zero in one of this run and the chunked run only: {shown}")
    return lines


@pytest.mark.parametrize("case,variant", RUNS, ids=[f"{c}-{v}" for c, v in RUNS])
def test_every_route_at_the_slab_limits(case, variant, poisoned):
    """Peak device memory: CASES' last column (V-under 19 GiB measured: bank 4, grad_value 4, the float-atomic /
    device-checked routes' fp32 image 8, workspace and the compare's fp64 temporaries; G-far the most, 23.5 GiB measured)."""
    import MultiScaleDeformableAttention as MSDA
    dtype, H, D = VARIANTS[variant]
    shapes, Nq, B, gib = CASES[case]
    need_memory(gib, f"{case} {variant}")
    v_over, g_over = slab_class(case)
    fwd_algos, bwd_routes = ONLY.get(variant, (FWD_ALGOS, tuple(r for r, _, _ in BWD_ROUTES)))
    fails, t0 = [], time.time()
    with released():
        x = device_inputs(case, variant, seed=RUNS.index((case, variant)))
        heads = selected_heads(H, seed=7)
        ref = Reference(x, heads, dtype)
        t_ref = time.time() - t0
        # ---- forward kernels
        ran_fwd, gather = {}, None
        for algo in ("gather",) + tuple(a for a in fwd_algos if a != "gather"):
            what = f"{case} {variant} fwd={algo}"
            out, launches = run_forward(MSDA, x, algo)
            if not torch.is_tensor(out):
                # a named kernel may refuse the KIND of the arguments (storage type, head width); never the size, never "auto"
                kind = algo in ("lds", "slices", "waves") and f"status {MSDA._E_UNSUPPORTED}" in out and not v_over
                ran_fwd[algo] = "refused (kind)" if kind else "ERROR"
                if not kind:
                    fails.append(f"{what}: {out}")
                continue
            ran_fwd[algo] = "+".join(launches)
            if algo == "gather":
                gather = out
            if v_over:
                # over the limit every forward is the row gather's flat-address kernel: bit-equal, and logged
                if not torch.equal(out, gather):
                    fails.append(f"{what}: not bit-equal to the row gather")
                want = ["msda_fwd_gather"] if algo in ("lds", "slices", "waves") else ["msda_fwd"]
                if launches != want:
                    fails.append(f"{what}: launched {launches}, not {want}")
            # (a flagged library call either runs the kernel its flag names or returns MMFS_E_UNSUPPORTED -- msda_capi.hip
            # tests *_supported and never falls back for a named flag --, and the shim re-routes by name only over the limit:
            # one "msda_fwd" launch that did not raise IS the named kernel.  The check below relies on that.)
            elif launches != ["msda_fwd"]:
                fails.append(f"{what}: a slab under the limit launched {launches}: the kernel asked for did not run")
            fails += ref.fails([out, None, None, None], H, what)
            fails += chunk_nets(MSDA, x, [out, None, None, None], dtype, what)
            if algo != "gather":
                del out
        if not v_over and dtype != torch.float32 and D == 128:
            # under the limit each named kernel runs itself (16-bit storage, D = 128: all three take the shape)
            for algo in ("lds", "slices", "waves"):
                if algo in fwd_algos and ran_fwd.get(algo) != "msda_fwd":
                    fails.append(f"{case} {variant} fwd={algo}: did not run its own kernel ({ran_fwd.get(algo)})")
        del gather
        # ---- backward routes
        ran_bwd = {}
        routes = [(r, c) for r, c, _ in BWD_ROUTES if r in bwd_routes]
        if v_over and dtype != torch.float32 and variant not in ONLY:
            routes.append(("taps=sorted", dict(register=True, taps="sorted")))      # by name: refused for the size, must not raise
        for route, cfg in routes:
            what = f"{case} {variant} bwd={route}"
            grads, ran = run_backward(MSDA, x, cfg)
            if not isinstance(grads, list):
                # (the LDS-levels taps kernel named for arguments of a kind it does not take -- fp32 storage -- raises,
                # as tests/test_level_geometry_gpu.py accepts; a refusal for the SIZE must not)
                kind = cfg.get("taps") == "lds" and f"status {MSDA._E_UNSUPPORTED}" in grads and dtype == torch.float32
                ran_bwd[route] = "refused (kind)" if kind else "ERROR"
                if not kind:
                    fails.append(f"{what}: {grads}")
                continue
            ran_bwd[route] = ran
            if route in ("sorted", "taps=sorted") and v_over and ran == "sorted":
                fails.append(f"{what}: the sorted route took a value slab over the limit")
            fails += ref.fails([None] + grads, H, what)
            fails += chunk_nets(MSDA, x, [None] + grads, dtype, what)
            del grads
            torch.cuda.empty_cache()
        secs = time.time() - t0
        print(f"\nLARGE-SLABS {case} {variant} P={points(case, dtype)} heads {heads}: reference {t_ref:.1f} s, test {secs:.1f} s, "
              f"peak {torch.cuda.max_memory_allocated() / GIB:.1f} GiB\n  fwd: " + " ".join(f"{a}={r}" for a, r in ran_fwd.items())
              + "\n  bwd: " + " ".join(f"{a}={r}" for a, r in ran_bwd.items())
              + "\n  worst ratios: " + " ".join(f"{n} {r:.3f}" for n, r in ref.worst.items()))
        torch.cuda.reset_peak_memory_stats()
        del x, ref
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:40])


# ------------------------------------------------------------------------------------------------- the fp8 bank
FP8_TABLES = {"under": [(256, 255), (15, 17)], "over": [(256, 256)]}      # S = 65535 / 65536 rows of 32768 bytes


@pytest.mark.parametrize("side", ["under", "over"])
def test_fp8_bank_forward_at_the_slab_limit(side, poisoned):
    """H = 256, D = 128 e4m3: a slab of 2^31 - 32768 bytes (buffer path) and of 2^31 (the flat path), forward only,
    against the dequantised bank at the selected heads.  Peak 8 GiB: the bf16 bank the quantiser reads 4, the fp8 bank 2,
    the compare ~1."""
    import MultiScaleDeformableAttention as MSDA
    need_memory(8, f"fp8 {side}")
    dtype, H, D, Nq, P = torch.bfloat16, 256, 128, 48, 2
    shapes = FP8_TABLES[side]
    with released():
        g = torch.Generator(device=DEV).manual_seed(21)
        sh, start = level_tables(shapes)
        S, L = int(sh.prod(1).sum()), sh.shape[0]
        assert (S * H * D > LIMIT) == (side == "over")
        bank = torch.rand(1, S, H, D, generator=g, device=DEV, dtype=dtype)
        q, scale = MSDA.quantize_bank_fp8(bank)
        del bank
        loc = (torch.rand(1, Nq, H, L, P, 2, generator=g, device=DEV) * 1.2 - 0.1).to(dtype)
        attn = torch.rand(1, Nq, H, L, P, generator=g, device=DEV) + 1e-5
        attn = (attn / attn.sum((-1, -2), keepdim=True)).to(dtype)
        heads = selected_heads(H, seed=8)
        idx = torch.as_tensor(heads, device=DEV)
        q_sub = q.index_select(2, idx).contiguous()
        s_sub = scale.view(1, H, D).index_select(1, idx).reshape(1, -1).contiguous()
        x = dict(value=MSDA.dequantize_bank_fp8(q_sub, s_sub, torch.float64), shapes=sh, start=start,
                 loc=loc.index_select(2, idx), attn=attn.index_select(2, idx),
                 grad=torch.zeros(1, Nq, len(heads) * D, device=DEV, dtype=torch.float64))
        x = {k: (v.double().cpu() if v.is_floating_point() else v) for k, v in x.items()}
        out = MSDA.ms_deform_attn_forward(q, sh.to(DEV), start.to(DEV), loc, attn, 1, value_scale=scale)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all())
        got = head_subset_outputs([out, None, None, None], heads, H)[0]
        rep = {}
        helpers.assert_within_bounds((got.double().cpu().numpy(), None, None, None), x, dtype, what=f"fp8 {side}",
                                     outputs=("out",), report=rep)
        print(f"\nLARGE-SLABS fp8 {side} S={S}: out {rep['out']:.3f} x the bound, peak {torch.cuda.max_memory_allocated() / GIB:.1f} GiB")
        torch.cuda.reset_peak_memory_stats()
        del q, scale, out, loc, attn


# ------------------------------------------------------------------------------------------------- the fused samplers
@pytest.mark.parametrize("side", ["under", "over"])
@pytest.mark.parametrize("variant", ["bf16", "fp32"])
def test_deform_sampler_at_the_slab_limit(variant, side, poisoned):
    """deform_sample_forward (plan -> sampler in one kernel, buffer-descriptor rows only): on V-under bit-equal to the plan
    kernel followed by the op's row gather -- what test_fused_sampler_walk_at_its_smallest asserts at small sizes --, with
    sample 1's slab starting past 2^31 bytes; on V-over it refuses (None: the module then takes plan + op).
    Peak 7 GiB: the bank 4 (under, N = 2), the op's output and the plan's tensors are small."""
    import MultiScaleDeformableAttention as MSDA
    from mmfs_amd.functions import DeformPlanFunction, deform_sample_forward
    from test_vit_adapter_gpu import plan_case
    need_memory(7, f"deform sampler {variant} {side}")
    dtype, H, D = VARIANTS[variant]
    shapes, Lq, N, _ = CASES["V-" + side]
    L, P = len(shapes), 4
    with released():
        c = plan_case(dtype, N, Lq, H, L, P, 2, 1, 1, seed=31)
        c["shapes"], c["start"] = level_tables(shapes, DEV)
        g = torch.Generator(device=DEV).manual_seed(32)
        value = torch.rand(N, int(c["shapes"].prod(1).sum()), H, D, device=DEV, generator=g, dtype=dtype)
        out = deform_sample_forward(value, c["shapes"], c["start"], c["both"], c["ref"], H, L, P)
        if side == "over":
            assert out is None
        else:
            assert out is not None
            loc, attn = DeformPlanFunction.apply(c["both"], c["ref"], c["shapes"], H, L, P)
            with knobs(MSDA, fwd="gather"):
                op = MSDA.ms_deform_attn_forward(value, c["shapes"], c["start"], loc, attn, 64)
            torch.cuda.synchronize()
            assert torch.equal(out, op) and bool(op[0].any()) and bool(op[1].any())
        del value, out, c


@pytest.mark.parametrize("side", ["under", "over"])
@pytest.mark.parametrize("variant", ["bf16", "fp32"])
def test_mmfs_sampler_at_the_slab_limit(variant, side, poisoned):
    """mmfs_sample_forward (MMFS's plan -> sampler kernel) likewise: bit-equal to plan kernel + row gather on V-under
    (two samples: the second one's slab starts past 2^31 bytes), None on V-over.  Peak 9 GiB (two samples' bank: 4 GiB,
    the plan's tensors and the outputs are small)."""
    import MultiScaleDeformableAttention as MSDA
    from mmfs_amd.functions.mmfs_plan_func import mmfs_sample_forward, sample_forward_groups
    from test_front_end_gpu import M_PLAN, N_PLAN, plan_forward, plan_inputs
    need_memory(9, f"MMFS sampler {variant} {side}")
    dtype, H, D = VARIANTS[variant]
    shapes, Lq = V_TABLES[side], 48
    n, L, P, N = 1, len(shapes), 4, N_PLAN
    with released():
        assert sample_forward_groups(dtype, Lq, D, n * L, P) == 1          # summed in sample order: bit-identical
        c = plan_inputs(dtype, n, L, Lq, Lq, N, H, P, "", seed=41)
        c["shapes"] = torch.tensor(shapes, device=DEV)
        dims = (N, Lq, H, L, P, n, M_PLAN, Lq, N)
        loc, attn, sink = plan_forward(dtype, c, dims, stacked=False)
        sh, st = level_tables(shapes, DEV)
        g = torch.Generator(device=DEV).manual_seed(42)
        value = torch.rand(N, int(sh.prod(1).sum()), H, D, device=DEV, generator=g, dtype=dtype)
        fused = mmfs_sample_forward(value, sh, st, *c["packed"], c["relpos"], c["ref"], c["ratios"], H, L, P)
        if side == "over":
            assert fused is None
        else:
            assert fused is not None
            with knobs(MSDA, fwd="gather"):
                op = MSDA.ms_deform_attn_forward(value, sh, st, loc, attn, 64)
            torch.cuda.synchronize()
            assert torch.equal(fused[0], op) and torch.equal(fused[1], sink) and bool(op[0].any()) and bool(op[1].any())
        del value, fused, c
