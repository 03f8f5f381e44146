"""The CLIP ViT's self-attention in fp64 on the STORED q, k, v and upstream gradient, with the error bounds of
csrc/mmfs_clip_attn.hip's header evaluated element by element (tests/test_clip_attn_gpu.py holds the kernels to them,
tests/test_clip_attn.py the framework's statement in T and four defective variants).

    r = clip64(q, k, v [B, L, H 64], heads, dtype, upstream=dO or None)

-> dict: ``context``, ``lse`` [B, H, L], ``dq``, ``dk``, ``dv``, ``E_<name>`` for each, and delta's shares ``S_dq``, ``S_dk``
[B, L, H].  The statement and its per-element bounds are qk_attn_refs.attention64's ``norm=None`` branch: plain attention of
heads of 64 channels for any number of queries and keys.  Nothing of that file had to be corrected: the framework's statement
in bf16 and fp16 meets every bound at every input of the GPU tests (tests/test_clip_attn.py measures it).

Rounding points the bounds assume: P and dS are rounded to T where they enter a product; lse and delta are fp32; the context
and dq, dk, dv are rounded once.  The framework's statement rounds more often; where it does, the bound counts its roundings.

The per-element bounds add absolute values where the errors of 64 channels and up to L keys largely cancel, so a second,
tight check goes with them: ``row_error``, llama_train_refs' measure for rows of 64 channels -- a row's error in the 2-norm
within TIGHT u of the row's norm plus delta's share plus a floor; llama_train_refs derives the factor.  u is UNIT of
llama_attn_refs (a whole unit in the last place: 2^-8 bf16, 2^-11 fp16), so TIGHT u is 8 2^-8 and 8 2^-11.
delta = rowsum(dO O) is formed from the STORED context, 64 products dO_c O_c with O rounded: its error has the size
D_j = |dO_j o O_j|_2 (times u / 2 rms) whatever the row's gradient is, and enters dq_j as p(j, .) k / 8 -- the p-weighted mean
key -- and dk_t as sum_j p(j, t) q_j / 8.  The shares are formed as llama_train_refs.train64 forms them, from fp64
quantities alone.  At L = 1 dq and dk are exactly 0 (p = 1, dP = delta) and the measure has no row to be relative to: it
applies from L = 2 on (the per-element bound covers L = 1).
"""
import torch

from llama_attn_refs import UNIT
from llama_train_refs import TIGHT, worst  # noqa: F401  (worst: the per-element ratio, shared)
from qk_attn_refs import attention64

D = 64
SCALE = 0.125
TIGHT_NAMES = ("context", "dq", "dk", "dv")
NAMES = ("context", "lse", "dq", "dk", "dv")


def heads_of(x, H):
    B, N, _ = x.shape
    return x.double().reshape(B, N, H, D).transpose(1, 2)               # [B, H, N, 64]


def clip64(q, k, v, heads, dtype, upstream=None):
    q, k, v = q.cpu(), k.cpu(), v.cpu()
    up = None if upstream is None else upstream.cpu()
    r = attention64(q, k, v, heads, norm=None, upstream=up, dtype=dtype)
    if up is None:
        return r
    p = r["p"]
    qh, kh, do, ctx = heads_of(q, heads), heads_of(k, heads), heads_of(up, heads), heads_of(r["context"], heads)
    Dj = (do * ctx).norm(dim=-1)                                        # [B, H, L]
    r["S_dq"] = (Dj * (p @ kh).norm(dim=-1) * SCALE).transpose(1, 2)    # [B, L, H]
    r["S_dk"] = ((p.pow(2).transpose(-1, -2) @ (Dj * qh.norm(dim=-1)).pow(2)[..., None]).squeeze(-1).sqrt() * SCALE).transpose(1, 2)
    return r


def row_error(got, ref, dtype, share=None):
    """worst |got_row - ref_row|_2 / (TIGHT u (|ref_row|_2 + share_row + 2^-6 R)) over the rows (a token of a head) of
    [B, L, H 64] tensors, R the rms of |ref_row|_2 over the tensor, ``share`` [B, L, H] or None; a non-finite entry of ``got``
    is Inf.  <= 1 passes."""
    ref = ref.double().cpu()
    got = got.detach().double().cpu().reshape(ref.shape)
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    B, L, C = ref.shape
    err = (got - ref).reshape(B, L, C // D, D).norm(dim=-1)
    size = ref.reshape(B, L, C // D, D).norm(dim=-1)
    R = float(size.pow(2).mean().sqrt())
    if share is not None:
        size = size + share
    return float((err / (TIGHT * UNIT[dtype] * (size + 2.0 ** -6 * R))).max())


def tight_ratios(got, ref, dtype):
    """{name: row_error} of context, dq, dk, dv (``got`` and ``ref`` dicts; ref from clip64)"""
    return {n: row_error(got[n], ref[n], dtype, ref.get("S_" + n)) for n in TIGHT_NAMES}


def bound_ratios(got, ref, names=NAMES):
    return {n: worst(got[n], ref[n], ref["E_" + n]) for n in names if n in got}


def draw(seed, L, dtype, B, H, device="cpu"):
    """the inputs of the GPU tests (tests/test_clip_attn_gpu.py) and of the yardstick that shows what the checks catch at
    exactly them (tests/test_clip_attn.py): unit-normal q, v, dO; k scaled by 1.5 and shifted by 0.25"""
    gen = torch.Generator().manual_seed(seed)
    q = torch.randn(B, L, H * D, generator=gen).to(device, dtype)
    k = (torch.randn(B, L, H * D, generator=gen) * 1.5 + 0.25).to(device, dtype)
    v = torch.randn(B, L, H * D, generator=gen).to(device, dtype)
    up = torch.randn(B, L, H * D, generator=gen).to(device, dtype)
    return q, k, v, up


# Two non-uniform score families for heads of 64 channels (tests/attn_score_families.py is wired to 128):
#   peaked   q scaled by 4: scores of deviation about 7 instead of 1.8, a row's weight on a handful of keys, a running
#            maximum that moves from tile to tile, whole tiles that underflow behind it;
#   sink     q shifted by 0.5 a channel and key 0 by 3: key 0's score is 64 (0.5) (3.25) / 8 = 13 on average against the other
#            keys' 1 +- 1.7, whose largest of some 300 lies near 6 -- key 0 leads a row by about 6 and holds most of its weight,
#            so dP - delta nearly cancels there.
FAMILIES = ("peaked", "sink")


def family(name, seed, L, dtype, B, H, device="cpu"):
    q, k, v, up = draw(seed, L, torch.float32, B, H)
    if name == "peaked":
        q = q * 4
    elif name == "sink":
        q = q + 0.5
        k[:, 0] += 3.0
    else:
        raise ValueError(name)
    return tuple(t.to(device, dtype) for t in (q, k, v, up))
