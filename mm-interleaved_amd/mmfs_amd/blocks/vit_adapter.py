"""The ViT-Adapter's interaction blocks -- the image encoder's callers of ``MSDeformAttn``
(mm_interleaved/models/encoders/vit_adapter/adapter_modules.py:15-233; 4 interaction blocks = 4 injectors +
6 extractors per ViT forward).  Constructor signatures and ``state_dict`` keys are the reference's, so its
checkpoints load with ``strict=True``; the ``attn`` of every block takes the fused front end
(``MSDeformAttn.fused_front_end``, csrc/msda_deform_plan.hip) and the depthwise convolution of ``ConvFFN`` runs on the
tokens as they lie, with its GELU (``DWConv.token_kernel``, csrc/msda_dwconv.hip).  LayerNorm, the Linear layers and
dropout are framework ops.

Differences from the reference, none of them in the numbers:
  * ``deform_inputs`` / ``get_reference_points`` build their tensors once per (image size, device) -- the level
    tables through ``levels.make_level_tables``, which also marks them as canonically packed for the op's backward --
    instead of six tensors per call;
  * stochastic depth is a module of this file (no ``timm`` import).

``AdapterPyramidHead`` is the stretch behind the blocks: from the adapter's tokens and the four ViT maps to the output
pyramid with its position tables, packed token-major as the feature bank reads it (csrc/mmfs_pyramid.hip).
"""
import math
from functools import partial

import torch
import torch.nn as nn
import torch.nn.functional as F
import torch.utils.checkpoint as cp

from ..functions.dwconv_func import DWConvTokensFunction, dwconv_tokens_supported
from ..functions.pyramid_func import PyramidHeadFunction, level_mask, level_sizes, pyramid_head_supported
from ..levels import cache_epoch, make_level_tables, tensor_version
from ..modules import MSDeformAttn

_ref_cache = {}
_inputs_cache = {}


def get_reference_points(spatial_shapes, device):
    """Pixel centres of the maps ``spatial_shapes`` [(H, W), ...], normalised to [0, 1], as (x, y):
    [1, sum H*W, 1, 2] fp32 -- one reference point per query, shared by the batch and by the levels.  Kept per
    (shapes, device)."""
    key = (tuple((int(h), int(w)) for h, w in spatial_shapes), str(torch.device(device)))
    hit = _ref_cache.get(key)
    if hit is not None:
        return hit
    # (kept tensors: built outside inference mode, see levels.make_level_tables)
    with torch.inference_mode(False), torch.no_grad():
        maps = []
        for h, w in key[0]:
            ys = torch.linspace(0.5, h - 0.5, h, dtype=torch.float32, device=device) / h
            xs = torch.linspace(0.5, w - 0.5, w, dtype=torch.float32, device=device) / w
            maps.append(torch.stack((xs[None, :].expand(h, w), ys[:, None].expand(h, w)), -1).reshape(1, h * w, 2))
        points = torch.cat(maps, 1)[:, :, None].contiguous()
    _ref_cache[key] = points
    return points


def deform_inputs(x):
    """x [B, C, h, w] (the image) -> ([reference_points, spatial_shapes, level_start_index] of the injector: the ViT's
    stride-16 tokens query the stride-8 / 16 / 32 pyramid;  the same three of the extractor: the pyramid's tokens query
    the stride-16 map).  The same tensor objects for every image of one size on one device."""
    h, w = int(x.shape[2]), int(x.shape[3])
    key = (h, w, str(x.device))
    hit = _inputs_cache.get(key)
    if hit is not None:
        return hit
    pyramid = [(h // 8, w // 8), (h // 16, w // 16), (h // 32, w // 32)]
    vit = [(h // 16, w // 16)]
    shapes1, start1, _ = make_level_tables(pyramid, 1, x.device)
    shapes2, start2, _ = make_level_tables(vit, 1, x.device)
    out = ([get_reference_points(vit, x.device), shapes1, start1],
           [get_reference_points(pyramid, x.device), shapes2, start2])
    _inputs_cache[key] = out
    return out


class DropPath(nn.Module):
    """Stochastic depth: in training a sample's residual branch is dropped with probability ``drop_prob`` and the
    kept ones are scaled by 1 / (1 - drop_prob); the identity in eval mode."""

    def __init__(self, drop_prob=0.0):
        super().__init__()
        self.drop_prob = float(drop_prob)

    def forward(self, x):
        if self.drop_prob == 0.0 or not self.training:
            return x
        keep = 1.0 - self.drop_prob
        mask = x.new_empty((x.shape[0],) + (1,) * (x.dim() - 1)).bernoulli_(keep)
        if keep > 0.0:
            mask.div_(keep)
        return x * mask

    def extra_repr(self):
        return f"drop_prob={self.drop_prob:.3f}"


class DWConv(nn.Module):
    """Depthwise 3x3 convolution of the pyramid's tokens: the 21 n tokens are the stride-8 map (16 n = 2H x 2W), the
    stride-16 map (4 n = H x W) and the stride-32 map (n), each convolved as an image with the same weights.

    ``token_kernel``: device tensors of one supported dtype, outside autocast, are convolved where they lie by
    ``DWConvTokensFunction`` (no transposed copies, no ``cat``); everything else -- CPU tensors, autocast, widths the
    16-byte lanes cannot take, mixed dtypes -- takes the reference's framework statement below.  The parameters stay
    inside the ``nn.Conv2d`` either way."""

    token_kernel = True

    def __init__(self, dim=768):
        super().__init__()
        self.dwconv = nn.Conv2d(dim, dim, 3, 1, 1, bias=True, groups=dim)

    def tokens(self, x, H, W, act):
        """The token kernel's result for ``act`` ("none" | "gelu"), or None when the route does not apply."""
        conv = self.dwconv
        if not (self.token_kernel and not torch.is_autocast_enabled() and x.dim() == 3
                and dwconv_tokens_supported(x, conv.weight, conv.bias)):
            return None
        level_hw = ((H * 2, W * 2), (H, W), (H // 2, W // 2))
        if sum(h * w for h, w in level_hw) != x.shape[1] or min(min(hw) for hw in level_hw) <= 0:
            return None
        return DWConvTokensFunction.apply(x, conv.weight, conv.bias, level_hw, act)

    def forward(self, x, H, W):
        out = self.tokens(x, H, W, "none")
        if out is not None:
            return out
        B, N, C = x.shape
        n = N // 21
        parts = []
        for lo, hi, (hh, ww) in ((0, 16 * n, (H * 2, W * 2)), (16 * n, 20 * n, (H, W)), (20 * n, N, (H // 2, W // 2))):
            img = x[:, lo:hi].transpose(1, 2).reshape(B, C, hh, ww)
            parts.append(self.dwconv(img).flatten(2).transpose(1, 2))
        return torch.cat(parts, 1)


class ConvFFN(nn.Module):
    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.):
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.dwconv = DWConv(hidden_features)
        self.act = act_layer()
        self.fc2 = nn.Linear(hidden_features, out_features)
        self.drop = nn.Dropout(drop)

    def forward(self, x, H, W):
        x = self.fc1(x)
        # convolution + exact GELU as one kernel call where the token kernel applies; dropout stays behind it
        a = self.dwconv.tokens(x, H, W, "gelu") if type(self.act) is nn.GELU and self.act.approximate == "none" else None
        x = self.drop(self.act(self.dwconv(x, H, W)) if a is None else a)
        return self.drop(self.fc2(x))


def _adapter_attn(dim, n_levels, num_heads, n_points, deform_ratio):
    attn = MSDeformAttn(d_model=dim, n_levels=n_levels, n_heads=num_heads, n_points=n_points, ratio=deform_ratio)
    attn.fused_front_end = True
    return attn


def _maybe_checkpoint(with_cp, fn, query, feat):
    if with_cp and query.requires_grad:
        return cp.checkpoint(fn, query, feat, use_reentrant=False)
    return fn(query, feat)


class Extractor(nn.Module):
    """Pyramid tokens (``query``) read the ViT's map (``feat``): query + attn, then the convolutional FFN."""

    def __init__(self, dim, num_heads=6, n_points=4, n_levels=1, deform_ratio=1.0, with_cffn=True, cffn_ratio=0.25,
                 drop=0., drop_path=0., norm_layer=partial(nn.LayerNorm, eps=1e-6), with_cp=False):
        super().__init__()
        self.query_norm = norm_layer(dim)
        self.feat_norm = norm_layer(dim)
        self.attn = _adapter_attn(dim, n_levels, num_heads, n_points, deform_ratio)
        self.with_cffn = with_cffn
        self.with_cp = with_cp
        if with_cffn:
            self.ffn = ConvFFN(in_features=dim, hidden_features=int(dim * cffn_ratio), drop=drop)
            self.ffn_norm = norm_layer(dim)
            self.drop_path = DropPath(drop_path) if drop_path > 0. else nn.Identity()

    def forward(self, query, reference_points, feat, spatial_shapes, level_start_index, H, W):
        def inner(query, feat):
            query = query + self.attn(self.query_norm(query), reference_points, self.feat_norm(feat), spatial_shapes,
                                      level_start_index, None)
            if self.with_cffn:
                query = query + self.drop_path(self.ffn(self.ffn_norm(query), H, W))
            return query

        return _maybe_checkpoint(self.with_cp, inner, query, feat)


class Injector(nn.Module):
    """ViT tokens (``query``) read the pyramid (``feat``): query + gamma * attn."""

    def __init__(self, dim, num_heads=6, n_points=4, n_levels=1, deform_ratio=1.0,
                 norm_layer=partial(nn.LayerNorm, eps=1e-6), init_values=0., with_cp=False):
        super().__init__()
        self.with_cp = with_cp
        self.query_norm = norm_layer(dim)
        self.feat_norm = norm_layer(dim)
        self.attn = _adapter_attn(dim, n_levels, num_heads, n_points, deform_ratio)
        self.gamma = nn.Parameter(init_values * torch.ones(dim), requires_grad=True)

    def forward(self, query, reference_points, feat, spatial_shapes, level_start_index):
        def inner(query, feat):
            return query + self.gamma * self.attn(self.query_norm(query), reference_points, self.feat_norm(feat),
                                                  spatial_shapes, level_start_index, None)

        return _maybe_checkpoint(self.with_cp, inner, query, feat)


class InteractionBlock(nn.Module):
    """Injector -> the ViT's own layers (``blocks``: modules called as ``blk(x, H, W)``) -> extractor(s)."""

    def __init__(self, dim, num_heads=6, n_points=4, norm_layer=partial(nn.LayerNorm, eps=1e-6), drop=0., drop_path=0.,
                 with_cffn=True, cffn_ratio=0.25, init_values=0., deform_ratio=1.0, extra_extractor=False,
                 with_cp=False):
        super().__init__()
        self.injector = Injector(dim=dim, n_levels=3, num_heads=num_heads, init_values=init_values, n_points=n_points,
                                 norm_layer=norm_layer, deform_ratio=deform_ratio, with_cp=with_cp)
        ext = partial(Extractor, dim=dim, num_heads=num_heads, n_points=n_points, norm_layer=norm_layer,
                      deform_ratio=deform_ratio, with_cffn=with_cffn, cffn_ratio=cffn_ratio, drop=drop,
                      drop_path=drop_path, with_cp=with_cp)
        self.extractor = ext(n_levels=1)
        self.extra_extractors = nn.Sequential(ext(), ext()) if extra_extractor else None

    def _inject(self, x, c, deform_inputs1):
        return self.injector(query=x, reference_points=deform_inputs1[0], feat=c, spatial_shapes=deform_inputs1[1],
                             level_start_index=deform_inputs1[2])

    def _extract(self, x, c, deform_inputs2, H, W):
        extractors = [self.extractor] + (list(self.extra_extractors) if self.extra_extractors is not None else [])
        for e in extractors:
            c = e(query=c, reference_points=deform_inputs2[0], feat=x, spatial_shapes=deform_inputs2[1],
                  level_start_index=deform_inputs2[2], H=H, W=W)
        return c

    def forward(self, x, c, blocks, deform_inputs1, deform_inputs2, H, W):
        x = self._inject(x, c, deform_inputs1)
        for blk in blocks:
            x = blk(x, H, W)
        return x, self._extract(x, c, deform_inputs2, H, W)


class InteractionBlockWithCls(InteractionBlock):
    """The same around a ViT with a class token: ``blocks`` is any callable on [cls | tokens] whose result has
    ``.last_hidden_state`` (the CLIP encoder's layers in the reference)."""

    def forward(self, x, c, cls, blocks, deform_inputs1, deform_inputs2, H, W):
        x = self._inject(x, c, deform_inputs1)
        x = blocks(torch.cat((cls, x), 1)).last_hidden_state
        cls, x = x[:, :1], x[:, 1:]
        return x, self._extract(x, c, deform_inputs2, H, W), cls


# ------------------------------------------------------------------ the output pyramid
_pos_cache = {}


def pyramid_pos_tables(pos_embed, H, W):
    """The position tables of the four output levels, fp32 [h_l * w_l, C] each: the reference's
    ``get_abs_pos(pos_embed[1:], h * w)`` (models/utils/pos_embed.py:16-40 as encoders/visual_tokenizer.py:74-82 calls
    it) -- the square table resized bicubically in fp32 to the level's side.  ``pos_embed`` is the [g * g, C] table, or
    the reference's parameter with its class-token row in front ([1 + g * g, C]; the row is dropped).  Built once per
    (table, H, W) on the table's device and kept until ``mmfs_amd.invalidate_caches()``.  The reference's resize knows square maps only: H == W."""
    if H != W:
        raise ValueError(f"position tables are defined for square maps only (H = {H}, W = {W})")
    # keyed like the package's other kept tensors (levels.py): pointer, version counter and the epoch that
    # ``mmfs_amd.invalidate_caches()`` moves; an entry keeps its table alive, so the address cannot be handed to another
    key = (pos_embed.data_ptr(), tensor_version(pos_embed), tuple(pos_embed.shape), pos_embed.dtype, str(pos_embed.device), H)
    hit = _pos_cache.get(key)
    if hit is not None and hit[0] is pos_embed and hit[1] == cache_epoch():
        return hit[2]
    # (kept tensors: built outside inference mode, see levels.make_level_tables)
    with torch.inference_mode(False), torch.no_grad():
        table = pos_embed.detach().float()
        n = table.shape[0]
        if math.isqrt(n) ** 2 != n and math.isqrt(n - 1) ** 2 == n - 1:
            table = table[1:]
        src = math.isqrt(table.shape[0])
        tabs = []
        for h, _ in level_sizes(H, W):
            if h == src:
                tabs.append(table.contiguous())
                continue
            t = F.interpolate(table.reshape(1, src, src, -1).permute(0, 3, 1, 2), size=(h, h), mode="bicubic",
                              align_corners=False)
            tabs.append(t.permute(0, 2, 3, 1).flatten(0, 2).contiguous())
        tabs = tuple(tabs)
    if len(_pos_cache) >= 16:
        _pos_cache.clear()
    _pos_cache[key] = (pos_embed, cache_epoch(), tabs)
    return tabs


class AdapterPyramidHead(nn.Module):
    """From the adapter's tokens to the output pyramid (vit_adapter_hf.py:137-153 and the position add of
    visual_tokenizer.py:74-82):
        c1 = adapter_up(c2) + c1 + bilinear x4 (x1),  c2 + bilinear x2 (x2),  c3 + x3,  c4 + bilinear x0.5 (x4),
    each plus its position table.  ``adapter_up`` is the reference's ``nn.ConvTranspose2d(dim, dim, 2, 2)`` with the
    reference's state-dict keys.

    forward(c, outs, c1, H, W, pos_embed=None, levels=(0, 1, 2, 3), packed=True):
      c      [B, 21 HW / 4, C]  the adapter's tokens c2 | c3 | c4 behind the last interaction block
      outs   four [B, HW, C]    the ViT's tokens behind each interaction block (the reference's ``outs`` before their
                                transposes); entries of levels that are not produced may be None
      c1     [B, C, 4H, 4W]     the spatial prior's first map, contiguous or channels_last (None without level 0)
      pos_embed                 None, the square sin-cos table (see ``pyramid_pos_tables``) or four ready tables
      levels                    which of (c1, c2, c3, c4) to produce, e.g. those whose side the decoder reads
    -> ``packed``: [B, sum h_l w_l, C], the levels one after the other, token-major -- what ``bank.llm_feature_bank`` and
    ``bank.pack_image_levels`` speak;  else the reference's list of [B, C, h_l, w_l] (on the kernel route views of the
    packed tensor).

    ``token_kernel``: device tensors of one supported dtype, outside autocast, take ``PyramidHeadFunction`` -- the
    transposed convolution becomes one GEMM on the c2 tokens (bias included; its parameter gradients are the GEMM's)
    and everything else one pass that reads each input once and writes the packed pyramid once.  CPU tensors, autocast,
    fp64, mixed dtypes and widths the 16-byte lanes cannot take run the reference's framework statement.  On by
    default (keep rule and measurements: DESIGN.md 4.13, profiles/vit_adapter.md)."""

    token_kernel = True

    def __init__(self, dim):
        super().__init__()
        self.adapter_up = nn.ConvTranspose2d(dim, dim, 2, 2)

    def up_tokens(self, c2):
        """adapter_up on the tokens of the 2H x 2W map: [B, n, C] -> [B, n, 4C] with columns (di, dj, o) -- output pixel
        (2i + di, 2j + dj), channel o, of token (i, j)."""
        w, b = self.adapter_up.weight, self.adapter_up.bias
        C = w.shape[0]
        w2 = w.permute(0, 2, 3, 1).reshape(C, 4 * w.shape[1])
        return torch.addmm(b.repeat(4), c2.reshape(-1, C), w2).view(c2.shape[0], c2.shape[1], w2.shape[1])

    def forward(self, c, outs, c1, H, W, pos_embed=None, levels=(0, 1, 2, 3), packed=True):
        levels = tuple(sorted(set(int(l) for l in levels)))
        mask = level_mask(levels)
        if mask == 0:
            raise ValueError("levels: at least one of 0..3")
        sizes = level_sizes(H, W)
        if pos_embed is None or isinstance(pos_embed, (tuple, list)):
            pos = None if pos_embed is None else tuple(pos_embed)
        else:
            pos = pyramid_pos_tables(pos_embed, H, W)
        outs = tuple(outs)
        if c.dim() != 3:
            raise ValueError(f"c: [B, 21 HW / 4, C] expected, got {tuple(c.shape)}")
        if pos is not None and any(t.device != c.device for l, t in enumerate(pos) if l in levels):
            raise ValueError(f"position tables on {pos[levels[0]].device}, tokens on {c.device}: move pos_embed to the tokens' device")
        B, _, C = c.shape
        if (self.token_kernel and not torch.is_autocast_enabled()
                and self.adapter_up.weight.dtype == c.dtype and self.adapter_up.weight.device == c.device
                and pyramid_head_supported(c, outs, c1, pos, H, W, mask)):
            up = self.up_tokens(c[:, :4 * H * W]) if mask & 1 else None
            out = PyramidHeadFunction.apply(c, *outs, up, c1, pos, H, W, mask)
            if packed:
                return out
            feats, lo = [], 0
            for l in levels:
                h, w = sizes[l]
                feats.append(out[:, lo:lo + h * w].transpose(1, 2).unflatten(2, (h, w)))
                lo += h * w
            return feats
        # the reference's statement
        n2, n3 = 4 * H * W, H * W
        img = lambda t, hw: t.transpose(1, 2).reshape(B, C, *hw).contiguous()     # noqa: E731
        feats = []
        for l in levels:
            if l == 0:
                f = self.adapter_up(img(c[:, :n2], sizes[1])) + c1
                f = f + F.interpolate(img(outs[0], sizes[2]), scale_factor=4, mode="bilinear", align_corners=False)
            elif l == 1:
                f = img(c[:, :n2], sizes[1]) + F.interpolate(img(outs[1], sizes[2]), scale_factor=2, mode="bilinear",
                                                             align_corners=False)
            elif l == 2:
                f = img(c[:, n2:n2 + n3], sizes[2]) + img(outs[2], sizes[2])
            else:
                f = img(c[:, n2 + n3:], sizes[3]) + F.interpolate(img(outs[3], sizes[2]), scale_factor=0.5,
                                                                  mode="bilinear", align_corners=False)
            if pos is not None:
                f = f + pos[l].to(f.dtype).reshape(*sizes[l], C).permute(2, 0, 1)
            feats.append(f)
        if packed:
            return torch.cat([f.flatten(2).transpose(1, 2) for f in feats], 1)
        return feats
