"""fp64 statement of the text loss (csrc/mmfs_text_loss.hip) on the stored logits, and next to it the per-element bounds
of that file's header.  Plain torch: runs on the CPU and on the device.  Every constant is the header's; none is fitted.

    e = 2^-24;  VEC = 16 bytes / sizeof(T);  n = 1 + ceil(floor(V / VEC) / 256) steps of a lane;  c = 6 + 3 combine steps
    D = sum_i p_i (M - x_i)              the p-weighted distance to the row's maximum M
    E_lse  = (2.5 D + 10 + 4 n + 5 c) e + V 2^-126 + 4 e |lse - M| + e |lse|
    E_loss = E_lse + e |loss|
    mean / sum of N rows: sum_r E_loss(r) / N + (ceil(rows / 1024) + 24) e sum_r |loss_r| / N
    grad:  u_T |ref| + t_T + |g| (p ((2.5 |x - lse| + 2) e + E_lse) + 5 e |p - [i == label]| + 2^-126)
"""
import math

import torch

from helpers import STORAGE_T, STORAGE_U

E24 = 2.0 ** -24
FLUSH = 2.0 ** -126             # v_exp_f32 flushes a denormal result
THREADS, COMBINE, REDUCE_THREADS = 256, 6 + 3, 1024


def lane_steps(V, dtype):
    vec = 16 // torch.empty(0, dtype=dtype).element_size()
    return 1 + math.ceil((V // vec) / THREADS)


def classes(labels, V, ignore_index):
    kept = labels != ignore_index
    inside = (labels >= 0) & (labels < V)
    return kept & inside, kept & ~inside


def rows64(x, labels, first=0, ignore_index=-100):
    """x [B, L, V] stored logits, labels [B, n] -> dict of fp64 tensors over the scored window: ``valid`` [B, n], ``lse``,
    ``loss`` (0 at rows that are not valid), ``p`` [B, n, V], ``onehot``, ``E_lse``, ``E_loss``"""
    B, L, V = x.shape
    n = labels.shape[1]
    xd = x.double()[:, first:first + n]
    valid, _ = classes(labels, V, ignore_index)
    M = xd.amax(-1)
    lse = torch.logsumexp(xd, -1)
    p = (xd - lse[..., None]).exp()
    D = torch.where(p > 0, p * (M[..., None] - xd), 0.0).sum(-1)
    at = labels.clamp(0, V - 1)
    loss = lse - xd.gather(-1, at[..., None]).squeeze(-1)
    onehot = torch.zeros_like(xd).scatter_(-1, at[..., None], 1.0)
    steps = lane_steps(V, x.dtype)
    E_lse = (2.5 * D + 10 + 4 * steps + 5 * COMBINE) * E24 + V * FLUSH + 4 * E24 * (lse - M).abs() + E24 * lse.abs()
    E_loss = E_lse + E24 * loss.abs()
    zero = torch.zeros_like(lse)
    return dict(valid=valid, xd=xd, lse=torch.where(valid, lse, zero), loss=torch.where(valid, loss, zero), p=p,
                onehot=onehot, E_lse=torch.where(valid, E_lse, zero), E_loss=torch.where(valid, E_loss, zero))


def reduced64(r, reduction):
    """-> (fp64 value, bound) of the "sum" / "mean" of ``rows64``'s result"""
    rows = r["loss"].numel()
    N = int(r["valid"].sum()) if reduction == "mean" else 1
    total = r["loss"].sum()
    if N == 0:
        return total / 0.0, torch.zeros(())
    chain = math.ceil(rows / REDUCE_THREADS) + 24
    return total / N, (r["E_loss"].sum() + chain * E24 * r["loss"].abs().sum()) / N


def grad64(r, g, shape, first, dtype):
    """g: the upstream of each scored row, fp64 [B, n] (mean: 1 / n_valid times the scalar's).  -> (ref, bound) [B, L, V]"""
    B, L, V = shape
    n = r["valid"].shape[1]
    live = r["valid"][..., None]
    gg = g[..., None].abs()
    diff = r["p"] - r["onehot"]
    ref_w = torch.where(live, diff * g[..., None], 0.0)
    dist = torch.where(r["p"] > 0, (r["xd"] - r["lse"][..., None]).abs(), 0.0)
    slack = gg * (r["p"] * ((2.5 * dist + 2) * E24 + r["E_lse"][..., None]) + 5 * E24 * diff.abs() + FLUSH)
    bound_w = torch.where(live, STORAGE_U[dtype] * ref_w.abs() + STORAGE_T[dtype] + slack, 0.0)
    ref = torch.zeros(shape, dtype=torch.float64, device=ref_w.device)
    bound = torch.zeros_like(ref)
    ref[:, first:first + n] = ref_w
    bound[:, first:first + n] = bound_w
    return ref, bound
