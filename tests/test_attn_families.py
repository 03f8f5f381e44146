"""Peaked, drifting and sink score rows (tests/attn_score_families.py) on the host, at exactly the inputs the GPU tests of the
LLaMA training, decode and prefill kernels draw: the families are what they claim; a host model of the kernels' rounding
points passes the row-wise measure (and the per-element bounds) there, so a kernel that misses it is wrong; and planted
defects of an online softmax -- no maximum, lse kept in T, an accumulator that is not rescaled, split partials merged without
their maxima -- are refused, where the unit-normal draws of the other tests let them pass."""
import functools
import math

import pytest
import torch

from attn_score_families import (CACHE_FAMILIES, TRAIN_FAMILIES, WALK_FAMILY, decode_case, describe, prefill_case, train_inputs)
from llama_attn_refs import SCALE, attend64, heads_of, merge
from llama_prefill_refs import clamped, hf_mask, left_padded
from llama_train_refs import TIGHT_NAMES, row_error, tight_ratios, train64, worst
from test_llama_train import kernel_model, statement

from mmfs_amd.functions.llama_attn_func import PREFILL_TILES, SPLIT_KEYS
from mmfs_amd.functions.llama_train_func import TRAIN_TILES
from mmfs_amd.llama_attn import rope_table

DTYPES = [torch.bfloat16, torch.float16]
ids = dict(ids=lambda d: str(d).split(".")[1] if isinstance(d, torch.dtype) else str(d).replace(" ", "_"))
B, H = 1, 2                                             # the GPU tests' training shape for the families
Q, K = TRAIN_TILES[:2]
L_FAMILY, L_WALK = 2 * Q + K // 2 + 3, 8 * Q + K + 5
MAX_POS = 2048
SEED = 5


@functools.lru_cache(maxsize=None)
def tables():
    return rope_table(128, MAX_POS)


@functools.lru_cache(maxsize=None)
def train_case(name, dtype, L=L_FAMILY):
    """inputs and the fp64 reference, made once and left unchanged"""
    x = train_inputs(name, SEED, L, dtype, B, H)
    cos, sin = tables()
    return x, train64(*x[:3], x[4], cos, sin, H, dtype, upstream=x[3])


def fmt(r):
    return ", ".join(f"{n} {x:.3g}" for n, x in r.items())


# ------------------------------------------------------------------ the inputs themselves
@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_the_families_are_what_they_claim(dtype):
    d = {name: describe(train_case(name, dtype)[1]) for name in TRAIN_FAMILIES + ("plain",)}
    for name, x in d.items():
        print(f"{name} {dtype}: lse {x['lse'][0]:.1f} .. {x['lse'][1]:.1f}, largest score {x['max_score']:.1f}, least rise of the row "
              f"maximum a key tile {x['tile_growth']:.1f}, dead key tiles {x['dead_tiles']}, key 0 at 50 .. 99.9 % in "
              f"{100 * x['sink_share_ok']:.1f} % of the rows")
    assert d["plain"]["max_score"] < 20 and abs(d["plain"]["lse"][1]) < 8       # what every other test draws
    assert d["rising 0.25"]["max_score"] > 89                                   # exp overflows in fp32 without the subtraction
    assert d["rising 0.25"]["tile_growth"] > 16
    assert d["falling 0.375"]["dead_tiles"] >= 1
    for name in ("sink 6", "sink 7"):
        assert d[name]["sink_share_ok"] >= 0.9, name


# ------------------------------------------------------------------ the host model passes
WALKS = [(WALK_FAMILY, L_WALK), ("plain", L_WALK)]


@pytest.mark.parametrize("dtype", DTYPES, **ids)
@pytest.mark.parametrize("case", [(n, L_FAMILY) for n in TRAIN_FAMILIES] + WALKS, ids=lambda c: f"{c[0]} L{c[1]}".replace(" ", "_"))
def test_the_kernel_model_passes_at_the_gpu_tests_inputs(case, dtype):
    name, L = case
    (q, k, v, do, pos), ref = train_case(name, dtype, L)
    cos, sin = tables()
    model = dict(zip(TIGHT_NAMES, kernel_model(q, k, v, do, pos, cos, sin, dtype, heads=H)))
    tight = tight_ratios(model, ref, dtype)
    loose = {m: worst(model[m], ref[m], ref["E_" + m]) for m in TIGHT_NAMES}
    print(f"model of the kernels' roundings, {name} L {L} {dtype}: row error {fmt(tight)}; per-element {fmt(loose)}")
    assert max(tight.values()) <= 1.0 and max(loose.values()) <= 1.0, (tight, loose)


# ------------------------------------------------------------------ planted defects
def softmax_model(q, k, v, do, dtype, defect=None, tile=K):
    """The kernels' rounding points at position 0 (the rotation is the identity there) with one defect of the softmax:
    ``no maximum``  p = exp(s) / sum exp(s) in fp32;  ``lse in T``  lse rounded to T before the backward's exp(s - lse);
    ``no rescale``  the forward as an online softmax over key tiles whose accumulator is not multiplied by alpha (l is).
    -> (context, dq, dk, dv) in T."""
    rt = lambda x: x.to(dtype).double()
    split = lambda x: x.double().unflatten(-1, (H, 128)).transpose(1, 2)
    join = lambda x: x.transpose(1, 2).flatten(2).to(dtype)
    qh, kh, vh, g = split(q), split(k), split(v), split(do)
    n = q.shape[1]
    future = torch.ones(n, n, dtype=torch.bool).triu(1)
    s = (qh @ kh.transpose(-1, -2) * SCALE).masked_fill(future, float("-inf"))
    if defect == "no maximum":
        e = s.float().exp()
        total = e.sum(-1, keepdim=True)
        p, lse = (e / total).double(), total.log().double()
    else:
        p, lse = s.softmax(-1), s.logsumexp(-1, keepdim=True)
    if defect == "no rescale":
        m = torch.full(s.shape[:-1] + (1,), float("-inf"), dtype=torch.float64)
        l, acc = torch.zeros_like(m), torch.zeros_like(qh)
        for k0 in range(0, n, tile):
            st = s[..., k0:k0 + tile]
            mn = torch.maximum(m, st.max(-1, keepdim=True).values)
            alpha, pt = (m - mn).exp(), (st - mn).exp()
            l = l * alpha + pt.sum(-1, keepdim=True)
            acc = acc + rt(pt) @ vh[..., k0:k0 + tile, :]                   # the defect: acc * alpha is missing
            m = mn
        ctx = rt(acc / l)
    else:
        ctx = rt(rt(p) @ vh)
    if defect == "lse in T":
        lse = rt(lse)
    pb = (s - lse).exp()
    ds = rt(pb * (g @ vh.transpose(-1, -2) - (g * ctx).sum(-1, keepdim=True)))
    return join(ctx), join(ds @ kh * SCALE), join(ds.transpose(-1, -2) @ qh * SCALE), join(rt(pb).transpose(-1, -2) @ g)


def refused(r):
    return (r["dq"] > 1.0 and r["dk"] > 1.0) or not all(math.isfinite(x) for x in r.values())


@pytest.mark.parametrize("dtype", DTYPES, **ids)
@pytest.mark.parametrize("name", TRAIN_FAMILIES, **ids)
def test_the_tight_check_refuses_planted_defects_at_every_family(name, dtype):
    """The three defects of tests/test_llama_train.py that position 0 can show, stated in fp64, at every family; the fourth,
    the inverse rotation with the forward's sign, is invisible here: at position 0 sin = 0 and both signs give g cos.
    ``falling 0.375`` (the parameter moved for the dead key tile) under the shifted mask: the key the shift lets in carries
    e^-0.53 of the weight of the one before it, dk moves in the first rows alone and measures 0.99 in bf16 (6.6 in fp16), so
    there the shift is held on the context, dq and dv (30, 4.2, 5.2); at the stated 0.25 it is held on dq and dk as everywhere."""
    (q, k, v, do, pos), ref = train_case(name, dtype)
    cos, sin = tables()
    x64 = tuple(t.double() for t in (q, k, v, do))
    model = softmax_model(q, k, v, do, dtype)                               # the model without a defect is the kernels' model
    r = tight_ratios(dict(zip(TIGHT_NAMES, model)), ref, dtype)
    assert max(r.values()) <= 1.0, r
    for defect in (dict(shift=1), dict(scaled=False), dict(with_delta=False)):
        got = dict(zip(TIGHT_NAMES, statement(*x64, pos, cos, sin, heads=H, **defect)))
        r = tight_ratios(got, ref, dtype)
        print(f"defect {defect} {name} {dtype}: row error {fmt(r)}")
        if name == "falling 0.375" and defect == dict(shift=1):
            assert r["context"] > 1.0 and r["dq"] > 1.0 and r["dv"] > 1.0, (defect, r)
        else:
            assert refused(r), (defect, r)
    plain, signed = statement(*x64, pos, cos, sin, heads=H), statement(*x64, pos, cos, sin, heads=H, forward_sign=True)
    assert all(torch.equal(a, b) for a, b in zip(plain, signed))


@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_the_softmax_defects_are_refused_at_rising_rows_and_pass_at_unit_normal_ones(dtype):
    """(a) no maximum: non-finite at ``rising 0.25`` (scores above 88.7).  (b) lse in T: moves p by u |lse|, 2 % at lse 6 and
    tens of percent at lse 50.  (c) no rescale: alpha is about 1 behind the first tile at unit-normal rows and e^-19 or less
    a tile at rising ones.  Each is printed at every family and at the plain draw, where (b) passes -- the gap these inputs close."""
    got = {}
    for name in TRAIN_FAMILIES + ("plain",):
        (q, k, v, do, pos), ref = train_case(name, dtype)
        if name == "plain":
            # the model has no rotation: the plain draw's own positions are replaced by 0 for this comparison
            cos, sin = tables()
            pos = torch.zeros_like(pos)
            ref = train64(q, k, v, pos, cos, sin, H, dtype, upstream=do)
        for defect in ("no maximum", "lse in T", "no rescale"):
            r = tight_ratios(dict(zip(TIGHT_NAMES, softmax_model(q, k, v, do, dtype, defect))), ref, dtype)
            got[name, defect] = r
            print(f"defect '{defect}' {name} {dtype}: row error {fmt(r)}")
    rising = TRAIN_FAMILIES[0]
    assert not all(math.isfinite(x) for x in got[rising, "no maximum"].values())
    assert max(got["plain", "no maximum"].values()) <= 1.0
    assert max(got["plain", "lse in T"].values()) <= 1.0                    # passes where every other test draws
    r = got[rising, "lse in T"]
    assert r["dq"] > 1.0 and r["dk"] > 1.0 and r["dv"] > 1.0, r
    r = got[rising, "no rescale"]
    assert r["context"] > 1.0 and refused(r), r


def test_the_model_is_linear_in_the_upstream_gradient_and_in_v():
    """bf16 only: its exponent range is fp32's, so 2^-20 dO keeps every dS normal; in fp16 dS goes subnormal at dO 2^-10
    already and no kernel can be held to this identity."""
    dtype = torch.bfloat16
    cos, sin = tables()
    for name in ("plain", TRAIN_FAMILIES[0]):
        (q, k, v, do, pos), _ = train_case(name, dtype)
        ctx, dq, dk, dv = kernel_model(q, k, v, do, pos, cos, sin, dtype, heads=H)
        for e in (-20, 20):
            f = 2.0 ** e
            scaled = lambda t: (t.double() * f).to(dtype)
            _, dq2, dk2, dv2 = kernel_model(q, k, v, scaled(do), pos, cos, sin, dtype, heads=H)
            for n, a, b in (("dq", dq, dq2), ("dk", dk, dk2), ("dv", dv, dv2)):
                assert torch.equal(scaled(a), b), (name, e, n)
            ctx2 = kernel_model(q, k, scaled(v), do, pos, cos, sin, dtype, heads=H)[0]
            assert torch.equal(scaled(ctx), ctx2), (name, e)


# ------------------------------------------------------------------ decode and prefill
def cache_model(q, keys, values, heads, dtype, mask=None, round_p=False, defect=None, split=SPLIT_KEYS):
    """The decode and prefill kernels' rounding points on the host: fp64 arithmetic on the stored q_rot (the rotation at position
    0 is exact), keys and values, the context rounded once; prefill rounds the unnormalised P to T where it enters the second
    product (``round_p``), decode keeps p in fp32 (csrc/mmfs_llama_attn.hip).  A masked key's score is the mask entry, as
    attend64 has it.  ``defect``: "merge": partials (m, l, o) of ``split`` keys summed without exp(m_j - M); "shifted": the
    weights of the keys one slot further on.  -> context [B, Lq, H 128] of T"""
    rt = lambda x: x.to(dtype).double()
    qh, kh, vh = heads_of(q, heads), keys.double(), values.double()
    s = qh @ kh.transpose(-1, -2) * SCALE
    if mask is not None:
        mb = mask.double().expand(s.shape[0], 1, s.shape[2], s.shape[3]).expand_as(s)
        s = torch.where(mb <= torch.finfo(dtype).min, mb, s + mb)
    if defect == "merge":
        o, l = torch.zeros_like(qh), torch.zeros(s.shape[:-1] + (1,), dtype=torch.float64)
        for k0 in range(0, s.shape[-1], split):
            e = (s[..., k0:k0 + split] - s[..., k0:k0 + split].max(-1, keepdim=True).values).exp()
            o, l = o + e @ vh[..., k0:k0 + split, :], l + e.sum(-1, keepdim=True)
        return merge(o / l).to(dtype)
    e = (s - s.max(-1, keepdim=True).values).exp()
    if defect == "shifted":
        e = e.roll(1, -1)
    return merge((rt(e) if round_p else e) @ vh / e.sum(-1, keepdim=True)).to(dtype)


def hold_cache_model(what, dtype, q, keys, values, mask, round_p, defects):
    r = attend64(q, keys, values, 3, mask=mask, dtype=dtype)
    model = cache_model(q, keys, values, 3, dtype, mask=mask, round_p=round_p)
    tight, loose = row_error(model, r["context"], dtype), worst(model, r["context"], r["E_context"])
    line = f"{what} {dtype}: model row error {tight:.3f}, per-element {loose:.3f}"
    assert tight <= 1.0 and loose <= 1.0, line
    for defect in defects:
        bad = row_error(cache_model(q, keys, values, 3, dtype, mask=mask, round_p=round_p, defect=defect), r["context"], dtype)
        line += f"; defect '{defect}' {bad:.3g}"
        assert bad > 1.0, line
    print(line)


@pytest.mark.parametrize("dtype", DTYPES, **ids)
@pytest.mark.parametrize("name", CACHE_FAMILIES + ("bias",), **ids)
def test_the_decode_model_passes_the_row_measure_and_two_defects_do_not(name, dtype):
    c = decode_case(name, dtype, SPLIT_KEYS)
    hold_cache_model(f"decode {name}", dtype, c["q"], c["keys"], c["values"], c["bias"], False, ("merge", "shifted"))


@pytest.mark.parametrize("dtype", DTYPES, **ids)
@pytest.mark.parametrize("name", CACHE_FAMILIES, **ids)
def test_the_prefill_model_passes_the_row_measure_and_a_shifted_key_does_not(name, dtype):
    c = prefill_case(name, dtype, PREFILL_TILES)
    n = c["held"] + c["Lq"]
    hf = clamped(hf_mask(left_padded(2, n, prefill_pads(n, c["held"])), c["Lq"], dtype), dtype)
    for kind, mask in (("none", None), ("row + causal", hf)):
        hold_cache_model(f"prefill {name} {kind}", dtype, c["q"], c["keys"], c["values"], mask, True, ("shifted",))


def prefill_pads(n, held):
    return min(n - 1, max(n // 3, held) + 1)            # tests/test_llama_prefill_gpu.py's pads_of
