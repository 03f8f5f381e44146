"""The image encoder's fused MSDeformAttn front end and the ViT-Adapter blocks on the GPU.

1. the plan kernels (csrc/msda_deform_plan.hip) element by element against the fp64 evaluation of the module's
   formulas, under derived bounds;  2. the fused sampler against the fp64 oracle on the plan kernel's own rounded
   locations / weights;  3. the module with ``fused_front_end`` on the committed encoder goldens at the bars of the
   unfused route;  4. the blocks against the reference's fixtures;  5. a forward + backward under graph capture."""
import ast

import numpy as np
import pytest
import torch

import helpers
from helpers import STORAGE_T, STORAGE_U, load_golden
from test_vit_adapter import CASES, OUTS, T, build, call, load_fixture, rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
CODE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


def lib():
    from mmfs_amd.functions import deform_plan_func
    return deform_plan_func._lib


def stream():
    return torch.cuda.current_stream().cuda_stream


def worst(got, ref, bound):
    """(worst |got - ref| / bound, its index, got, ref, bound there); inf for an element that is not finite (an unwritten, poisoned one)."""
    err = (got.double() - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0))
    ratio = torch.where(torch.isfinite(got.double()), ratio, float("inf"))
    k = int(ratio.argmax())
    where = tuple(int(v) for v in np.unravel_index(k, tuple(ratio.shape)))
    return (float(ratio.flatten()[k]), where, float(got.flatten()[k]), float(ref.expand_as(ratio).flatten()[k]),
            float(bound.expand_as(ratio).flatten()[k]))


def plan_case(dtype, N, Lq, H, L, P, R, Nr, Lref, seed):
    """Inputs of one plan problem: T-rounded heads in ONE [N, Lq, C] tensor (offsets' columns first) plus packed
    copies, reference points, level table; and the fp64 evaluation of the formulas on them."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    n_off = H * L * P * 2
    C = n_off + H * L * P
    both = torch.empty(N, Lq, C, device=DEV, dtype=torch.float32)
    both[..., :n_off] = torch.randn(N, Lq, n_off, device=DEV, generator=g) * 2.0
    both[..., n_off:] = torch.rand(N, Lq, C - n_off, device=DEV, generator=g) * 16.0 - 8.0        # |logit| <= 8
    both = both.to(dtype)
    ref = torch.rand(Nr, Lq, Lref, R, device=DEV, generator=g)
    if R == 4:
        ref[..., 2:] = ref[..., 2:] * 0.3 + 0.05
    shapes = torch.randint(1, 41, (L, 2), device=DEV, generator=g)
    off = both[..., :n_off].double().view(N, Lq, H, L, P, 2)
    logit = both[..., n_off:].double().view(N, Lq, H, L, P)
    r = ref.double().expand(N, Lq, L, R)[:, :, None, :, None, :]                                  # [N, Lq, 1, L, 1, R]
    if R == 2:
        scale = 1.0 / torch.stack((shapes[:, 1], shapes[:, 0]), -1).double()[None, None, None, :, None, :]
        scale = scale.expand(N, Lq, 1, L, 1, 2)
    else:
        scale = r[..., 2:] * 0.5 / P
    attn = torch.softmax(logit.reshape(N, Lq, H, L * P), -1).view(N, Lq, H, L, P)
    return dict(both=both, ref=ref, shapes=shapes, off=off, logit=logit, point=r[..., :2], scale=scale, attn=attn,
                loc=r[..., :2] + off * scale, n_off=n_off, C=C)


PLAN_GRID = [(L, R, Nr_is_N, Lref_is_L, stacked) for L in (1, 2, 3, 8) for R in (2, 4) for Nr_is_N in (False, True)
             for Lref_is_L in (False, True) for stacked in (False, True)]


@pytest.mark.parametrize("P", [2, 4, 8])
@pytest.mark.parametrize("dtype", DTYPES)
def test_plan_kernels_element_by_element(dtype, P, monkeypatch):
    """Plan forward and backward against the fp64 formulas, every element under its own bound (u = the storage type's
    rounding, t its subnormal floor):
        |attn - ref|       <= u ref + 2^-17 ref + t
        |loc - ref|        <= u |ref| + 2^-22 (|ref point| + |scaled offset|) + t
        |grad_logit - ref| <= u |ref| + 2^-17 a_i (|g_i| + sum_j a_j |g_j|) + t
        |grad_off - ref|   <= u |ref| + 2^-22 |ref| + t
    Every bound carries the subnormal floor t, not the weights' alone: a result of a few 1e-6 (a small weight's
    gradient, a location next to 0 where point and offset cancel) is an fp16 subnormal, where ONE correct rounding is
    off by up to half the subnormal spacing (2^-25), not by u |ref| -- the derivation without it holds for normal
    results only (seen: fp16, P = 2, boxes, a location of ~1e-5 at 1.75 x the bound without t); for fp32 / bf16 the
    term is below 2^-133 and changes nothing.
    Outputs are allocated poisoned: an element no lane writes is NaN and fails."""
    helpers.poison_allocations(monkeypatch)
    u, t = STORAGE_U[dtype], STORAGE_T[dtype]
    N, Lq, H = 2, 37, 4             # (H even: the stacked rows stay multiples of the kernels' 16-byte accesses at P = 2)
    es = torch.empty(0, dtype=dtype).element_size()
    f_fwd, f_bwd = lib().mmfs_deform_plan_forward, lib().mmfs_deform_plan_backward
    report = {}
    for i, (L, R, nr_n, lref_l, stacked) in enumerate(PLAN_GRID):
        Nr, Lref = (N if nr_n else 1), (L if lref_l else 1)
        c = plan_case(dtype, N, Lq, H, L, P, R, Nr, Lref, seed=1000 * P + i)
        n_off, C = c["n_off"], c["C"]
        dims = (N, Lq, H, L, P, Nr, Lref, R)
        if stacked:
            off_t, att_t, ld = c["both"], None, (C, C)
            off_ptr, att_ptr = off_t.data_ptr(), off_t.data_ptr() + n_off * es
        else:
            off_t, att_t, ld = c["both"][..., :n_off].contiguous(), c["both"][..., n_off:].contiguous(), (0, 0)
            off_ptr, att_ptr = off_t.data_ptr(), att_t.data_ptr()
        loc = torch.empty(N, Lq, H, L, P, 2, device=DEV, dtype=dtype)
        attn = torch.empty(N, Lq, H, L, P, device=DEV, dtype=dtype)
        rc = f_fwd(CODE[dtype], off_ptr, att_ptr, ld[0], ld[1], c["ref"].data_ptr(), c["shapes"].data_ptr(),
                   loc.data_ptr(), attn.data_ptr(), *dims, stream())
        assert rc == 0, rc
        what = f"L={L} P={P} R={R} Nr={Nr} Lref={Lref} stacked={stacked}"
        res = {"attn": worst(attn, c["attn"], u * c["attn"] + 2.0 ** -17 * c["attn"] + t),
               "loc": worst(loc, c["loc"], u * c["loc"].abs()
                            + 2.0 ** -22 * (c["point"].abs() + (c["off"] * c["scale"]).abs()) + t)}
        # backward: the saved weights are the storage type's numbers, as the forward leaves them
        g = torch.Generator(device=DEV).manual_seed(77 + i)
        a = c["attn"].to(dtype)
        g_attn = torch.randn(a.shape, device=DEV, generator=g).to(dtype)
        g_loc = torch.randn(loc.shape, device=DEV, generator=g).to(dtype)
        if stacked:
            d_both = torch.empty(N, Lq, C, device=DEV, dtype=dtype)
            go_ptr, ga_ptr = d_both.data_ptr(), d_both.data_ptr() + n_off * es
        else:
            d_off = torch.empty(N, Lq, n_off, device=DEV, dtype=dtype)
            d_att = torch.empty(N, Lq, C - n_off, device=DEV, dtype=dtype)
            go_ptr, ga_ptr = d_off.data_ptr(), d_att.data_ptr()
        rc = f_bwd(CODE[dtype], g_loc.data_ptr(), g_attn.data_ptr(), a.data_ptr(), c["ref"].data_ptr(),
                   c["shapes"].data_ptr(), go_ptr, ga_ptr, ld[0], ld[1], *dims, stream())
        assert rc == 0, rc
        if stacked:
            d_off, d_att = d_both[..., :n_off], d_both[..., n_off:]
        a64, ga64 = a.double(), g_attn.double()
        dot = (a64 * ga64).sum((-1, -2), keepdim=True)
        dot_abs = (a64 * ga64.abs()).sum((-1, -2), keepdim=True)
        ref_gl = a64 * (ga64 - dot)
        ref_go = g_loc.double() * c["scale"]
        res["grad_logit"] = worst(d_att.reshape(a.shape), ref_gl,
                                  u * ref_gl.abs() + 2.0 ** -17 * a64 * (ga64.abs() + dot_abs) + t)
        res["grad_off"] = worst(d_off.reshape(loc.shape), ref_go, u * ref_go.abs() + 2.0 ** -22 * ref_go.abs() + t)
        for n, v in res.items():
            report[n] = max(report.get(n, 0.0), v[0])
        bad = {n: v for n, v in res.items() if not v[0] <= 1.0}
        assert not bad, f"{what} {dtype}: bound broken: {bad}"
    print(f"PLAN-BOUNDS {str(dtype)[6:]} P={P} worst ratios " + " ".join(f"{n} {v:.3f}" for n, v in report.items()))


def sampler_case(dtype, shapes, P, R, D, N, Lq, H, seed):
    L = len(shapes)
    c = plan_case(dtype, N, Lq, H, L, P, R, 1 if R == 2 else N, 1 if R == 2 else L, seed)
    sh, st = helpers.level_tables(shapes, DEV)
    c["shapes"], c["start"] = sh, st
    g = torch.Generator(device=DEV).manual_seed(seed + 1)
    c["value"] = torch.rand(N, int(sh.prod(1).sum()), H, D, device=DEV, generator=g).to(dtype)
    return c


SAMPLER_TABLES = [  # the level tables of the committed encoder goldens and of the adapter fixtures, with their P / R
    ([(8, 8), (4, 4), (2, 2)], 4, 2), ([(4, 4)], 4, 2), ([(5, 3), (2, 4)], 2, 4),
    ([(16, 16), (8, 8), (4, 4)], 4, 2), ([(8, 8)], 4, 2)]


@pytest.mark.parametrize("D", [16, 32, 64])
@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_sampler_against_the_oracle_on_the_plans_own_numbers(dtype, D, monkeypatch):
    from mmfs_amd.functions import DeformPlanFunction, deform_sample_forward
    helpers.poison_allocations(monkeypatch)
    report = {}
    for i, (shapes, P, R) in enumerate(SAMPLER_TABLES):
        N, Lq, H, L = 2, 150, 3, len(shapes)
        c = sampler_case(dtype, shapes, P, R, D, N, Lq, H, seed=500 + 10 * i + D)
        loc, attn = DeformPlanFunction.apply(c["both"], c["ref"], c["shapes"], H, L, P)
        out = deform_sample_forward(c["value"], c["shapes"], c["start"], c["both"], c["ref"], H, L, P)
        assert out is not None and out.shape == (N, Lq, H * D) and out.dtype == dtype
        torch.cuda.synchronize()
        x = dict(value=c["value"].double().cpu(), shapes=c["shapes"].cpu(), start=c["start"].cpu(),
                 loc=loc.double().cpu(), attn=attn.double().cpu(), grad=torch.zeros(N, Lq, H * D, dtype=torch.float64))
        helpers.assert_within_bounds((out.double().cpu().numpy(), None, None, None), x, dtype,
                                     what=f"sampler {shapes} P={P} R={R} D={D}", outputs=("out",), report=report)
    print(f"SAMPLER-BOUNDS {str(dtype)[6:]} D={D} worst ratio {report.get('out', 0.0):.3f}")
    # an empty batch: no launch, an empty result
    c = sampler_case(dtype, [(4, 4)], 4, 2, D, 0, 5, 3, seed=9)
    out = deform_sample_forward(c["value"], c["shapes"], c["start"], c["both"], c["ref"], 3, 1, 4)
    assert out is not None and out.shape == (0, 5, 3 * D)
    # head rows the gather cannot take: the caller is told to run plan + op
    c = sampler_case(dtype, [(4, 4)], 4, 2, 24, 1, 5, 3, seed=9)
    assert deform_sample_forward(c["value"], c["shapes"], c["start"], c["both"], c["ref"], 3, 1, 4) is None


SAMPLER_WALKS = [(torch.float32, 16, "4 lanes per query: the 8 samples are one chunk"), (torch.bfloat16, 32, "4 lanes, 16-bit rows"),
                 (torch.bfloat16, 16, "2 lanes: chunks of 4 samples, two per query")]


@pytest.mark.parametrize("live,R", [(1, 2), (2, 2), (3, 4), (4, 2), (5, 4), (8, 2)])
@pytest.mark.parametrize("dtype,D,what", SAMPLER_WALKS, ids=[f"{str(w[0])[6:]}-D{w[1]}" for w in SAMPLER_WALKS])
def test_fused_sampler_walk_at_its_smallest(dtype, D, what, live, R, monkeypatch):
    """deform_sample_fwd's walk over a chunk's live tap records where each branch is alone, equal bit for bit to the plan
    kernel followed by the op's row gather: three queries (a ragged tile; the workgroup's other waves hold no query at
    all and walk nothing) of one head with 8 samples each (levels 3 x 5 and 2 x 2, P = 4), of which the first ``live``
    keep their logit and the others get -1e4 -- a softmax weight of exactly 0 in every storage type, so their taps are
    not walked: the odd prologue alone, the pair without the loop, one loop trip, every tap."""
    import MultiScaleDeformableAttention as MSDA
    from mmfs_amd.functions import DeformPlanFunction, deform_sample_forward
    helpers.poison_allocations(monkeypatch)
    N, Lq, H, L, P = 2, 3, 1, 2, 4
    c = sampler_case(dtype, [(3, 5), (2, 2)], P, R, D, N, Lq, H, seed=900 + live)
    c["both"][..., c["n_off"] + live:] = -1e4
    loc, attn = DeformPlanFunction.apply(c["both"], c["ref"], c["shapes"], H, L, P)
    w = attn.reshape(N, Lq, L * P)
    assert not bool(w[..., live:].any()) and bool(w[..., :live].all())
    old, MSDA._fwd_algo = MSDA._fwd_algo, "gather"
    try:
        op = MSDA.ms_deform_attn_forward(c["value"], c["shapes"], c["start"], loc, attn, 64)
    finally:
        MSDA._fwd_algo = old
    out = deform_sample_forward(c["value"], c["shapes"], c["start"], c["both"], c["ref"], H, L, P)
    assert out is not None, what
    assert torch.equal(out, op) and bool(op.any()), what


# ------------------------------------------------------------------ the module on the committed encoder goldens
def enc_module(name, dtype):
    from mmfs_amd.modules import MSDeformAttn
    z = load_golden(name)
    m = MSDeformAttn(**ast.literal_eval(str(z["cfg"])))
    m.load_state_dict({k[len("param."):]: T(v, torch.float32) for k, v in z.items() if k.startswith("param.")}, strict=True)
    m = m.to(DEV, dtype)
    m.fused_front_end = True
    args = lambda q, f, ref: (q, ref, f, T(z["spatial_shapes"], None, DEV), T(z["level_start_index"], None, DEV),   # noqa: E731
                              T(z["padding_mask"], None, DEV) if "padding_mask" in z else None)
    return z, m, args


class Routes:
    """Counts which front end a module call took."""

    def __init__(self, monkeypatch):
        import mmfs_amd.modules.ms_deform_attn as mod
        self.plan = self.sampler = self.softmax = 0
        real_plan, real_sampler, real_softmax = mod.DeformPlanFunction, mod.deform_sample_forward, mod.F.softmax
        outer = self

        class Plan:
            @staticmethod
            def apply(*a):
                outer.plan += 1
                return real_plan.apply(*a)

        def sampler(*a):
            outer.sampler += 1
            return real_sampler(*a)

        def softmax(*a, **k):
            outer.softmax += 1
            return real_softmax(*a, **k)

        monkeypatch.setattr(mod, "DeformPlanFunction", Plan)
        monkeypatch.setattr(mod, "deform_sample_forward", sampler)
        monkeypatch.setattr(mod.F, "softmax", softmax)

    def take(self):
        r = (self.plan, self.sampler, self.softmax)
        self.plan = self.sampler = self.softmax = 0
        return r


@pytest.mark.parametrize("name", ["enc_injector", "enc_extractor", "enc_boxes_padded"])
@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-5), (torch.float16, 2e-3), (torch.bfloat16, 1.6e-2)])
def test_module_fused_route_on_the_encoder_goldens(name, dtype, tol, monkeypatch):
    """``fused_front_end = True`` at the bars test_modules_gpu.py holds for the unfused route: outputs 2e-5 / 2e-3 /
    1.6e-2, fp32 gradients 1e-4 (every parameter); no-grad calls through plan + op and through the fused sampler at
    the same output bars; reference points that need a gradient take the framework route and get it."""
    z, m, args = enc_module(name, dtype)
    routes = Routes(monkeypatch)
    q = T(z["query"], dtype, DEV).requires_grad_(True)
    f = T(z["feat"], dtype, DEV).requires_grad_(True)
    ref = T(z["reference_points"], dtype, DEV)
    out = m(*args(q, f, ref))
    assert routes.take() == (1, 0, 0)
    e_out = rel(out, z["out"])
    assert out.dtype == dtype and e_out <= tol, e_out
    out.backward(T(z["grad_out"], dtype, DEV))
    if dtype == torch.float32:
        errs = {"query": rel(q.grad, z["grad_query"]), "feat": rel(f.grad, z["grad_feat"])}
        errs.update({k: rel(p.grad, z["grad." + k]) for k, p in m.named_parameters()})
        print(f"MODULE-FUSED {name} fp32 out {e_out:.2e} worst grad {max(errs.values()):.2e}")
        assert all(v <= 1e-4 for v in errs.values()), errs
    m.eval()
    with torch.no_grad():
        assert m.fused_sampler is True                 # the default for calls without gradients: the fused sampler
        m.fused_sampler = False
        o1 = m(*args(q, f, ref))
        assert routes.take() == (1, 0, 0)              # ... and plan + op behind the attribute
        m.fused_sampler = True
        o2 = m(*args(q, f, ref))
        o3 = m(*args(q, f, ref))                       # (second call: the kept stacked weights)
        assert routes.take() == (0, 2, 0)
    e1, e2 = rel(o1, z["out"]), rel(o2, z["out"])
    print(f"MODULE-FUSED {name} {str(dtype)[6:]} out {e_out:.2e} no-grad plan+op {e1:.2e} sampler {e2:.2e}")
    assert e1 <= tol and e2 <= tol and torch.equal(o2, o3)
    # a reference_points tensor that requires a gradient: framework ops, and the gradient arrives
    m.train()
    ref_g = ref.clone().requires_grad_(True)
    out = m(*args(q, f, ref_g))
    assert routes.take() == (0, 0, 1)
    assert rel(out, z["out"]) <= tol
    out.backward(T(z["grad_out"], dtype, DEV))
    assert ref_g.grad is not None and torch.isfinite(ref_g.grad).all() and float(ref_g.grad.abs().max()) > 0


# ------------------------------------------------------------------ the blocks against the reference's fixtures
def gpu_block(name, z, dtype, **over):
    m, sd = build(name, z, **over)
    m.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)
    return m.to(DEV, dtype)


@pytest.mark.parametrize("name", CASES)
def test_blocks_fp32_against_the_reference(name, monkeypatch):
    """Outputs within 2e-5, input and parameter gradients within 1e-4 of the largest reference entry (the project's
    bars for the encoder module), through the fused front end."""
    z = load_fixture(name)
    routes = Routes(monkeypatch)
    m = gpu_block(name, z, torch.float32).train()
    xs = {k[len("in."):]: T(v, torch.float32, DEV).requires_grad_(True) for k, v in z.items() if k.startswith("in.")}
    outs = call(name, m, z, xs, torch.float32, DEV)
    n_attn = sum(1 for mod in m.modules() if type(mod).__name__ == "MSDeformAttn")
    assert routes.take() == (n_attn, 0, 0)
    e_out = {n: rel(o, z["out." + n]) for n, o in zip(OUTS[name], outs)}
    torch.autograd.backward(list(outs), [T(z["grad_out." + n], torch.float32, DEV) for n in OUTS[name]])
    e_in = {k: rel(x.grad, z["grad_in." + k]) for k, x in xs.items()}
    e_par = {k: rel(p.grad, z["grad." + k]) for k, p in m.named_parameters()}
    print(f"BLOCK-FP32 {name} out {max(e_out.values()):.2e} grad_in {max(e_in.values()):.2e} grad_param {max(e_par.values()):.2e}")
    assert all(v <= 2e-5 for v in e_out.values()), e_out
    assert all(v <= 1e-4 for v in e_in.values()), e_in
    assert all(v <= 1e-4 for v in e_par.values()), e_par


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("dtype,tag", [(torch.bfloat16, "bf16"), (torch.float16, "fp16")])
def test_blocks_16bit_forward_against_the_references_own_error(name, dtype, tag, monkeypatch):
    """Forward outputs only; the bar is twice the error of the reference's own 16-bit CPU run of the same block
    against its fp64 run (``ref_err.<dtype>.<output>`` of the fixture; the factor two: GEMM and sum orders differ
    between CPU and GPU).  16-bit gradients are not held to the fixture -- the reference's own differ from its fp64
    ones by 20-75 % (a rounded location changes the sampled cell); the plan's gradients are held per element above,
    the op's by its own tests."""
    z = load_fixture(name)
    routes = Routes(monkeypatch)
    m = gpu_block(name, z, dtype).eval()
    xs = {k[len("in."):]: T(v, dtype, DEV) for k, v in z.items() if k.startswith("in.")}
    with torch.no_grad():
        outs = call(name, m, z, xs, dtype, DEV)
    n_attn = sum(1 for mod in m.modules() if type(mod).__name__ == "MSDeformAttn")
    assert routes.take() == (0, n_attn, 0)             # no-grad calls: the fused sampler
    errs = {n: (rel(o, z["out." + n]), 2.0 * float(z[f"ref_err.{tag}.{n}"])) for n, o in zip(OUTS[name], outs)}
    print(f"BLOCK-16BIT {name} {tag} " + " ".join(f"{n} {e:.2e} (bar {b:.2e})" for n, (e, b) in errs.items()))
    assert all(o.dtype == dtype for o in outs)
    assert all(e <= b for e, b in errs.values()), errs


def test_with_cp_gives_the_same_outputs_and_gradients_on_the_gpu():
    name = "adapter_interaction_cls"
    z = load_fixture(name)
    res = []
    for with_cp in (False, True):
        m = gpu_block(name, z, torch.float32, with_cp=with_cp).train()
        xs = {k[len("in."):]: T(v, torch.float32, DEV).requires_grad_(True) for k, v in z.items() if k.startswith("in.")}
        outs = call(name, m, z, xs, torch.float32, DEV)
        torch.autograd.backward(list(outs), [T(z["grad_out." + n], torch.float32, DEV) for n in OUTS[name]])
        res.append(([o.detach() for o in outs], {k: x.grad for k, x in xs.items()}, {k: p.grad for k, p in m.named_parameters()}))
    (o0, i0, p0), (o1, i1, p1) = res
    assert all(torch.equal(a, b) for a, b in zip(o0, o1))
    for k in i0:
        assert rel(i1[k], i0[k].double().cpu().numpy()) <= 1e-5, k
    for k in p0:
        assert rel(p1[k], p0[k].double().cpu().numpy()) <= 1e-5, k


# ------------------------------------------------------------------ graph capture
def test_injector_forward_backward_replays_from_a_graph():
    """One forward + backward of an Injector on the fused route, captured and replayed: bit-equal to the eager call."""
    from mmfs_amd.blocks import deform_inputs
    z = load_fixture("adapter_injector")
    m = gpu_block("adapter_injector", z, torch.float32).train()
    h, w = (int(v) for v in z["image_hw"])
    d1, _ = deform_inputs(torch.zeros(1, 3, h, w, device=DEV))
    q = T(z["in.query"], torch.float32, DEV).requires_grad_(True)
    f = T(z["in.feat"], torch.float32, DEV).requires_grad_(True)
    grad = T(z["grad_out.out"], torch.float32, DEV)
    params = list(m.parameters())

    def step():
        out = m(q, d1[0], f, d1[1], d1[2])
        return (out,) + torch.autograd.grad(out, [q, f] + params, grad)

    want = [t.detach().clone() for t in step()]
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
    print("GRAPH-REPLAY max |replay - eager| " + " ".join(f"{n} {v:.1e}" for n, v in diffs.items() if v > 0) or "all 0")
    assert all(torch.isfinite(a).all() for a in captured)
    assert all(v == 0.0 for v in diffs.values()), {n: v for n, v in diffs.items() if v > 0}
