"""Score rows at which an online softmax can go wrong, for the four fused attention kernels' tests.

The tests' usual draw (q ~ N(0, 1), k ~ 1.5 N(0, 1) + 0.25) gives diffuse softmax rows: the running maximum settles in the
first key tile, ``alpha`` is 1 afterwards, nothing under- or overflows and |lse| stays below 8.  A family replaces eight
channels of every head (``SLOW``: 60..63 and 124..127) in q by 2.0 and in key t by one number ``kv(t)``, so that the score
gains the part 8 . 2 . kv / sqrt(128) = 1.414 kv on top of the random part of the other 120 channels:

    ``rising a``    kv(t) = floor(8 a t) / 8     the row maximum rises at every key tile (alpha far below 1), scores pass 88.7
    ``falling a``   kv(t) = -floor(8 a t) / 8    the maximum is set by the first keys, later tiles underflow to 0
    ``sink a``      kv(t) = a at the sink slots (key 0 unless told otherwise), else 0: one key holds most of a row's weight
    ``plain``       nothing is changed

Every large-score family is drawn at position 0 (the rotary table's row cos = 1, sin = 0), where the rotation is exact: at
real positions the rounding of q_rot and k_rot moves a score of 50 by tenths, and fp64 on the stored inputs is then no
reference a kernel's roundings can be held to row by row (a host model of them fails the tight measure by 1.3 .. 2.7).
The rotation at real positions is what the plain draws hold.

    family(name, q, k, L)                  q, k [B, L, H 128] fp32 -> (q, k) with the family applied, before the cast to T
    cache_family(name, keys, sinks=(0,))   keys [.., H, n, 128] fp32 (a cache image) -> keys with kv(t) in slot t
    slow_queries(q)                        q [.., H 128] -> q with the SLOW channels at 2.0
    train_inputs(name, seed, L, dtype, ..) llama_train_refs.draw with the family applied: (q, k, v, dO, positions)
    decode_inputs / prefill_inputs         the decode and prefill tests' tensors on the host
    describe(ref)                          what the tests assert about a training reference's rows themselves

Parameters that were moved so that ``describe``'s conditions hold at the training tests' L = 291 (the conditions stayed):
``falling`` 0.25 -> 0.375 for the whole key tile below 2^-126 (at 0.25 the key tile 192..255 still holds p of 1e-30); 0.25
stays a family of its own, because the steeper the fall, the less a mask shifted by one key changes (the key it lets in
carries e^(-1.414 a) of its neighbour's weight), and that planted defect is held on dq and dk at 0.25 as at every other family.
``sink`` 4 and 6 -> 6 and 7 (at 4 key 0 holds half of the weight or more in 39 % of the rows only)."""
import math

import torch

from llama_attn_refs import D
from llama_train_refs import draw

SLOW = (60, 61, 62, 63, 124, 125, 126, 127)
Q_SLOW = 2.0
PART = len(SLOW) * Q_SLOW / math.sqrt(D)                # the score's large part is PART . kv(t)
TRAIN_FAMILIES = ("rising 0.25", "falling 0.25", "falling 0.375", "sink 6", "sink 7")
WALK_FAMILY = "rising 0.0625"
CACHE_FAMILIES = ("rising 0.125", "falling 0.125", "sink 6")
TILE = 64                                               # describe's key tile


def parse(name):
    kind, _, a = name.partition(" ")
    assert kind in ("rising", "falling", "sink", "plain"), name
    return kind, float(a) if a else 0.0


def profile(name, n, sinks=(0,)):
    """kv(t) for t < n, fp32 [n]"""
    kind, a = parse(name)
    t = torch.arange(n, dtype=torch.float32)
    if kind == "sink":
        kv = torch.zeros(n)
        kv[list(sinks)] = a
        return kv
    steps = torch.floor(8 * a * t) / 8
    return steps if kind == "rising" else -steps


def _slow_index(heads):
    return torch.tensor([h * D + c for h in range(heads) for c in SLOW])


def slow_queries(q):
    q = q.clone()
    q[..., _slow_index(q.shape[-1] // D)] = Q_SLOW
    return q


def family(name, q, k, L, sinks=(0,)):
    if parse(name)[0] == "plain":
        return q, k
    assert q.dtype == torch.float32 and k.dtype == torch.float32 and q.shape[1] == L == k.shape[1]
    k = k.clone()
    k[..., _slow_index(k.shape[-1] // D)] = profile(name, L, sinks)[None, :, None]
    return slow_queries(q), k


def cache_family(name, keys, sinks=(0,)):
    if parse(name)[0] == "plain":
        return keys
    assert keys.dtype == torch.float32 and keys.shape[-1] == D
    keys = keys.clone()
    keys[..., list(SLOW)] = profile(name, keys.shape[-2], sinks)[:, None]
    return keys


def train_inputs(name, seed, L, dtype, B, H, device="cpu", first=5):
    """the training tests' draw (llama_train_refs.draw) with the family applied in fp32 and every position 0; ``plain`` keeps
    draw's own positions"""
    q, k, v, up, pos = draw(seed, L, torch.float32, B, H, first=first)
    if parse(name)[0] != "plain":
        q, k = family(name, q, k, L)
        pos = torch.zeros_like(pos)
    return tuple(t.to(device, dtype) for t in (q, k, v, up)) + (pos.to(device),)


def rising_bias(n, dtype, step=0.25):
    """an fp32 bias row [1, 1, 1, n] that rises by ``step`` a key, at values T holds (the framework route casts it to T)"""
    return (step * torch.arange(n, dtype=torch.float32)).to(dtype).float()[None, None, None]


def decode_inputs(name, dtype, kv, B, H, sinks, seed):
    """One decode step onto kv - 1 held keys: the family lies in the cache's rows and in the new token's key (slot kv - 1),
    the query's SLOW channels are 2.0, the position is 0.  ``name`` = "bias": plain unit-normal keys and queries for the
    run with a rising bias.  -> dict of host tensors: q, k, v [B, 1, H 128] of T, keys, values [B, H, kv, 128] of T (all kv
    logical rows: the first kv - 1 go into the cache, the last one is k / v again)"""
    gen = torch.Generator().manual_seed(seed)
    keys = torch.randn(B, H, kv, D, generator=gen) * 1.5 + 0.25
    values = torch.randn(B, H, kv, D, generator=gen)
    q = torch.randn(B, 1, H * D, generator=gen)
    if name != "bias":
        keys, q = cache_family(name, keys, sinks), slow_queries(q)
    keys, values, q = keys.to(dtype), values.to(dtype), q.to(dtype)
    token = lambda rows: rows[:, :, -1:].transpose(1, 2).reshape(B, 1, H * D).contiguous()
    return {"q": q, "k": token(keys), "v": token(values), "keys": keys, "values": values}


def prefill_inputs(name, dtype, held, Lq, B, H, sinks, seed):
    """A chunk of Lq tokens behind ``held`` ones, the family over all held + Lq keys -> q, k, v [B, Lq, H 128], keys, values
    [B, H, held + Lq, 128] of T on the host (the last Lq logical rows are k / v again)"""
    n = held + Lq
    gen = torch.Generator().manual_seed(seed)
    keys = torch.randn(B, H, n, D, generator=gen) * 1.5 + 0.25
    values = torch.randn(B, H, n, D, generator=gen)
    q = torch.randn(B, Lq, H * D, generator=gen)
    keys, q = cache_family(name, keys, sinks), slow_queries(q)
    keys, values, q = keys.to(dtype), values.to(dtype), q.to(dtype)
    tokens = lambda rows: rows[:, :, held:].transpose(1, 2).reshape(B, Lq, H * D).contiguous()
    return {"q": q, "k": tokens(keys), "v": tokens(values), "keys": keys, "values": values}


def decode_case(name, dtype, split_keys):
    """the decode tests' case ``name`` (a member of CACHE_FAMILIES, or "bias"): B = 2, H = 3, kv = 2 split_keys + 1, the sink at
    slot 0 and once more in the middle split; "bias" adds ``bias``, the rising fp32 row [1, 1, 1, kv]"""
    kv = 2 * split_keys + 1
    order = CACHE_FAMILIES + ("bias",)
    case = decode_inputs(name, dtype, kv, 2, 3, (0, split_keys + 7), 4000 + order.index(name))
    case["bias"] = rising_bias(kv, dtype) if name == "bias" else None
    return case


def prefill_case(name, dtype, tiles):
    """the prefill tests' case: B = 2, H = 3, held = K + 1, Lq = 2 G + 1 of the kernel's tiles (W, G, K), the sink at slot 0 and
    once more among the appended tokens, in the second query tile"""
    _, G, K = tiles
    held, Lq = K + 1, 2 * G + 1
    case = prefill_inputs(name, dtype, held, Lq, 2, 3, (0, held + G + 7), 5000 + CACHE_FAMILIES.index(name))
    case["held"], case["Lq"] = held, Lq
    return case


def describe(ref, tile=TILE, rows_from=TILE, last_rows=128):
    """What a training reference (train64's dict: ``p`` [B, H, L, L] and ``lse``, causal) says about its own rows:

    ``max_score``        the largest live score (fp32's exp overflows above 88.7)
    ``tile_growth``      the smallest rise of a row's maximum from one key tile of ``tile`` to the next, over every row and every
                         pair of consecutive tiles the row sees whole
    ``dead_tiles``       key tiles, wholly live for all of the last ``last_rows``-row query tile's rows, where every p of those
                         rows is below 2^-126
    ``sink_share_ok``    the share of rows j >= ``rows_from`` in which key 0 holds between 50 % and 99.9 % of the weight
    ``lse``              (min, max)"""
    p, lse = ref["p"], ref["lse"]
    L = p.shape[-1]
    live = torch.ones(L, L, dtype=torch.bool).tril()
    s = torch.where(live, p.clamp_min(1e-300).log() + lse[..., None], torch.full_like(p, float("-inf")))
    out = {"max_score": float(s.max()), "lse": (float(lse.min()), float(lse.max()))}
    growth = float("inf")
    for c in range(L // tile - 1):
        rows = slice((c + 2) * tile - 1, L)                                 # rows that see tiles c and c + 1 whole
        a = s[..., rows, c * tile:(c + 1) * tile].max(-1).values
        b = s[..., rows, (c + 1) * tile:(c + 2) * tile].max(-1).values
        growth = min(growth, float((b - a).min()))
    out["tile_growth"] = growth
    q0 = (L - 1) // last_rows * last_rows
    out["dead_tiles"] = sum(1 for c in range(q0 // tile) if float(p[..., q0:, c * tile:(c + 1) * tile].max()) < 2.0 ** -126)
    w0 = p[..., rows_from:, 0]
    out["sink_share_ok"] = float(((w0 >= 0.5) & (w0 <= 0.999)).double().mean()) if L > rows_from else float("nan")
    return out
