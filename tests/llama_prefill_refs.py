"""What the prefill tests share (csrc/mmfs_llama_prefill.hip): HF's prompt mask as the reference builds it, and a host
model of the kernel's tile walk.  The fp64 statement and the bounds are tests/llama_attn_refs.py's ``attend64`` with
n = held + Lq keys; it is handed the mask clamped at finfo(T).min (it treats -Inf as -Inf)."""
import torch

D = 128
LOG2E = 1.44269504088896340736
SKIP_MARGIN = 1024.0


def hf_mask(attention, Lq, dtype):
    """HF's ``_prepare_decoder_attention_mask`` for Lq new tokens behind held ones: attention [B, held + Lq] of 0 / 1 ->
    ``_expand_mask + _make_causal_mask`` [B, 1, Lq, held + Lq] in T.  Where a padded key is also a future key the sum of
    two finfo.min is -Inf."""
    Bm, n = attention.shape
    low = torch.finfo(dtype).min
    causal = torch.cat((torch.zeros(Lq, n - Lq, dtype=dtype), torch.full((Lq, Lq), low, dtype=dtype).triu(1)), dim=-1)
    inverted = 1.0 - attention[:, None, None, :].expand(Bm, 1, Lq, n).to(dtype)
    expanded = inverted.masked_fill(inverted.to(torch.bool), low)
    return expanded + causal[None, None]


def padding_row(attention, dtype):
    """the padding part alone, [B, 1, 1, kv]: with the kernel's causal flag it is the mask above"""
    inverted = 1.0 - attention[:, None, None, :].to(dtype)
    return inverted.masked_fill(inverted.to(torch.bool), torch.finfo(dtype).min)


def clamped(mask, dtype):
    return None if mask is None else mask.double().clamp_min(torch.finfo(dtype).min)


def left_padded(batch, n, pads):
    """attention [batch, n]: row 1 starts with ``pads`` padded keys"""
    attention = torch.ones(batch, n)
    attention[1, :pads] = 0
    return attention


def tile_walk(q_rot, keys, values, heads, held, mask, dtype, tiles, causal=False, skip=True):
    """The kernel's order of operations on the host: query tiles of tiles[1] rows, key tiles of tiles[2], fp32, one running
    (m, l, O) per row, p rounded to T where it enters the second product, the skip rule.  q_rot [B, Lq, H 128],
    keys / values [B, H, n, 128] of T, mask [B or 1, 1, Lq or 1, n] or None -> (context [B, Lq, H 128] of T, tiles visited)"""
    _, G, K = tiles
    B, Lq, _ = q_rot.shape
    n = keys.shape[2]
    low = torch.tensor(torch.finfo(dtype).min, dtype=torch.float32)
    scale = torch.tensor(0.08838834764831845, dtype=torch.float32)
    qh = q_rot.float().reshape(B, Lq, heads, D).transpose(1, 2)             # [B, H, Lq, 128]
    kf, vf = keys.float(), values.float()
    out = torch.empty(B, heads, Lq, D, dtype=dtype)
    ninf = torch.tensor(float("-inf"))
    visited = 0
    for b in range(B):
        bias_b = None if mask is None else mask[b if mask.shape[0] > 1 else 0, 0].float().expand(Lq, n)
        for q0 in range(0, Lq, G):
            rows = torch.arange(q0, min(q0 + G, Lq))
            for h in range(heads):
                m = torch.full((len(rows),), float("-inf"))
                l = torch.zeros(len(rows))
                O = torch.zeros(len(rows), D)
                for k0 in range(0, n, K):
                    t = torch.arange(k0, min(k0 + K, n))
                    may = skip and bool(m.min() - low >= SKIP_MARGIN)
                    if causal and k0 > held + int(rows[-1]) and may:
                        break
                    bias = torch.zeros(len(rows), len(t)) if bias_b is None else bias_b[rows][:, t]
                    masked = bias <= low
                    if causal:
                        masked = masked | (t[None, :] > held + rows[:, None])
                    eff = torch.where(bias != bias, torch.tensor(float("inf")), torch.where(masked, low, bias))
                    if may and bool(eff.max() <= low):
                        continue
                    visited += 1
                    s = torch.where(masked, low, (qh[b, h, rows] @ kf[b, h, t].T) * scale + bias)
                    mn = torch.maximum(m, s.max(dim=1).values)
                    base = torch.where(mn == ninf, torch.zeros(()), mn)
                    alpha = torch.exp2((m - base) * LOG2E)
                    p = torch.exp2((s - base[:, None]) * LOG2E)
                    l = l * alpha + p.sum(dim=1)
                    O = O * alpha[:, None] + p.to(dtype).float() @ vf[b, h, t]
                    m = mn
                out[b, h, rows] = (O / l[:, None]).to(dtype)
    return out.transpose(1, 2).reshape(B, Lq, heads * D), visited
