"""The vision transformer of the reference's main path (vit_tt.py: TTAttention, TTMlp, TTBlock, TTVisionTransformer and
the `tt{m,r}_` / `tk{m,r}_` factories), without timm: what the reference inherits from timm 0.4.x (PatchEmbed, DropPath,
Attention.forward, Mlp.forward, Block.forward, VisionTransformer) is restated here.  State-dict keys and the shapes of the
dense parts are timm's, so a DeiT / ViT checkpoint loads as it does there.

The attention body runs through `functional.self_attention` on the three column slices of the packed qkv projection,
read in place; the step between the branches -- proj_drop / drop, DropPath, the residual add and the next LayerNorm --
through `functional.add_layer_norm` (csrc/prenorm.hip: one launch forward, two backward).  `linear` is one of
TTLinearM / TTLinearR / TKLinearM / TKLinearR and builds the projections whose weight name is in `hp_dict.ranks`; the
others are nn.Linear.  Nothing is ever downloaded: a dense state dict comes from `dense_dict=` or a local file."""
from functools import partial

import torch
import torch.nn as nn

from . import functional as HF
from ._layer_common import _local_state_dict, create_model  # noqa: F401 (_local_state_dict: the name stays importable here)
from .tk_layers import TKLinearM, TKLinearR
from .tt_layers import TTLinearM, TTLinearR


class DropPath(nn.Module):
    """timm's stochastic depth per sample: x.div(keep_prob) * floor(keep_prob + rand((B, 1, ..., 1))) in training."""

    def __init__(self, drop_prob=None):
        super().__init__()
        self.drop_prob = drop_prob

    def forward(self, x):
        if not self.drop_prob or not self.training:
            return x
        keep_prob = 1.0 - self.drop_prob
        shape = (x.shape[0],) + (1,) * (x.dim() - 1)
        return x.div(keep_prob) * (keep_prob + torch.rand(shape, dtype=x.dtype, device=x.device)).floor_()


class PatchEmbed(nn.Module):
    """Image to patch tokens: a strided convolution `proj`, flattened and transposed to (B, patches, embed_dim)."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=768, norm_layer=None):
        super().__init__()
        img_size = (img_size, img_size) if isinstance(img_size, int) else tuple(img_size)
        patch_size = (patch_size, patch_size) if isinstance(patch_size, int) else tuple(patch_size)
        self.img_size, self.patch_size = img_size, patch_size
        self.grid_size = (img_size[0] // patch_size[0], img_size[1] // patch_size[1])
        self.num_patches = self.grid_size[0] * self.grid_size[1]
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=patch_size, stride=patch_size)
        self.norm = norm_layer(embed_dim) if norm_layer else nn.Identity()

    def forward(self, x):
        B, C, H, W = x.shape
        if (H, W) != self.img_size:
            raise ValueError(f"PatchEmbed: input image size ({H}*{W}) doesn't match model ({self.img_size[0]}*{self.img_size[1]})")
        return self.norm(self.proj(x).flatten(2).transpose(1, 2))


def _projection(linear, hp_dict, dense_dict, name, in_features, out_features, bias=True):
    w_name, b_name = name + 'weight', name + 'bias'
    if hp_dict is not None and w_name in hp_dict.ranks:
        return linear(in_features, out_features, bias=bias, hp_dict=hp_dict, name=w_name,
                      dense_w=None if dense_dict is None else dense_dict[w_name],
                      dense_b=None if dense_dict is None or not bias else dense_dict[b_name])
    return nn.Linear(in_features, out_features, bias=bias)


class TTAttention(nn.Module):
    """vit_tt.py:33-61 with timm's Attention.forward: one packed qkv projection, softmax(q k^T / sqrt(d)) v per head,
    `proj`.  `proj_drop` is kept as a module and applied by the caller's tail (TTBlock), not here."""

    def __init__(self, dim, num_heads=8, qkv_bias=False, attn_drop=0., proj_drop=0., linear=TTLinearM, block_id=None,
                 hp_dict=None, dense_dict=None):
        super().__init__()
        if dim % num_heads:
            raise ValueError(f"TTAttention: dim {dim} is not a multiple of num_heads {num_heads}")
        self.num_heads = num_heads
        self.scale = (dim // num_heads) ** -0.5
        pre = 'blocks.' + str(block_id) + '.attn.'
        self.qkv = _projection(linear, hp_dict, dense_dict, pre + 'qkv.', dim, dim * 3, qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = _projection(linear, hp_dict, dense_dict, pre + 'proj.', dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)
        self.route = None                       # None: the measured rule; "launch" / "composed" force a route

    def forward(self, x):
        C = x.shape[-1]
        qkv = self.qkv(x)
        ctx, _ = HF.self_attention(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], None, self.num_heads,
                                   dropout_p=self.attn_drop.p, training=self.training, need_scores=False,
                                   route=self.route)
        return self.proj(ctx)


class TTMlp(nn.Module):
    """vit_tt.py:64-94 with timm's Mlp.forward: fc1, act, drop, fc2.  The second `drop` is applied by the caller's tail."""

    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.,
                 linear=TTLinearM, block_id=None, hp_dict=None, dense_dict=None):
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        pre = 'blocks.' + str(block_id) + '.mlp.'
        self.fc1 = _projection(linear, hp_dict, dense_dict, pre + 'fc1.', in_features, hidden_features)
        self.act = act_layer()
        self.fc2 = _projection(linear, hp_dict, dense_dict, pre + 'fc2.', hidden_features, out_features)
        self.drop = nn.Dropout(drop)

    def forward(self, x):
        return self.fc2(self.drop(self.act(self.fc1(x))))


def _affine_layer_norm(m):
    return isinstance(m, nn.LayerNorm) and m.elementwise_affine and m.bias is not None and len(m.normalized_shape) == 1


class TTBlock(nn.Module):
    """vit_tt.py:97-111 with timm's Block.forward: x + drop_path(attn(norm1(x))), then x + drop_path(mlp(norm2(x))).

    `forward(x)` returns the new stream.  `forward(x, normed, next_norm)` is the chained form: `normed` is norm1(x) where
    the caller has it already; with `next_norm` (the LayerNorm that reads this block's output: the next block's norm1,
    or the model's final norm) the return value is (stream, next_norm(stream)), both from one `add_layer_norm`.  A norm
    layer that is not an affine nn.LayerNorm is composed plainly."""

    def __init__(self, dim, num_heads, mlp_ratio=4., qkv_bias=False, drop=0., attn_drop=0., drop_path=0.,
                 act_layer=nn.GELU, norm_layer=nn.LayerNorm, linear=TTLinearM, block_id=None, hp_dict=None,
                 dense_dict=None):
        super().__init__()
        self.norm1 = norm_layer(dim)
        self.attn = TTAttention(dim, num_heads=num_heads, qkv_bias=qkv_bias, attn_drop=attn_drop, proj_drop=drop,
                                linear=linear, block_id=block_id, hp_dict=hp_dict, dense_dict=dense_dict)
        self.drop_path = DropPath(drop_path) if drop_path > 0. else nn.Identity()
        self.norm2 = norm_layer(dim)
        self.mlp = TTMlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop,
                         linear=linear, block_id=block_id, hp_dict=hp_dict, dense_dict=dense_dict)
        self.route = None                       # of the two tails; the attention has its own

    def set_route(self, route):
        """Forces one route (None, "launch", "composed") on the attention and both tails; returns self."""
        self.route = self.attn.route = route
        return self

    def _tail(self, x, branch, drop, norm):
        """(x + drop_path(drop(branch)), norm(that sum))"""
        if _affine_layer_norm(norm):
            p_path = self.drop_path.drop_prob if isinstance(self.drop_path, DropPath) else 0.0
            return HF.add_layer_norm(x, branch, norm.weight, norm.bias, eps=norm.eps, dropout_p=drop.p,
                                     drop_path_p=p_path or 0.0, training=self.training, route=self.route)
        x = x + self.drop_path(drop(branch))
        return x, norm(x)

    def forward(self, x, normed=None, next_norm=None):
        if normed is None:
            normed = self.norm1(x)
        x, normed = self._tail(x, self.attn(normed), self.attn.proj_drop, self.norm2)
        branch = self.mlp(normed)
        if next_norm is None:
            return x + self.drop_path(self.mlp.drop(branch))
        return self._tail(x, branch, self.mlp.drop, next_norm)


def _trunc_normal_(t, std=.02):
    return nn.init.trunc_normal_(t, std=std, a=-2.0, b=2.0)


class TTVisionTransformer(nn.Module):
    """vit_tt.py:114-131 with timm 0.4.x's VisionTransformer: patch embedding, class (and distillation) token, position
    embedding, `depth` TTBlocks with the linspace DropPath schedule, the final LayerNorm (eps 1e-6) and the head(s).
    `forward_features` chains the blocks: each block's second tail also computes the next block's norm1 (the final norm
    for the last block).  As in the reference, timm's initialisation (truncated normal of std 0.02) reaches the tokens,
    the position embedding and the head; the blocks keep the initialisation of their own layers."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, num_classes=1000, embed_dim=768, depth=12, num_heads=12,
                 mlp_ratio=4., qkv_bias=True, representation_size=None, distilled=False, drop_rate=0., attn_drop_rate=0.,
                 drop_path_rate=0., norm_layer=None, act_layer=None, linear=TTLinearM, hp_dict=None, dense_dict=None):
        super().__init__()
        if representation_size is not None:
            raise NotImplementedError("TTVisionTransformer: representation_size (timm's pre_logits layer) is not "
                                      "restated here; none of the reference's factories uses it")
        self.num_classes = num_classes
        self.num_features = self.embed_dim = embed_dim
        self.num_tokens = 2 if distilled else 1
        norm_layer = norm_layer or partial(nn.LayerNorm, eps=1e-6)
        act_layer = act_layer or nn.GELU
        self.patch_embed = PatchEmbed(img_size=img_size, patch_size=patch_size, in_chans=in_chans, embed_dim=embed_dim)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.dist_token = nn.Parameter(torch.zeros(1, 1, embed_dim)) if distilled else None
        self.pos_embed = nn.Parameter(torch.zeros(1, self.patch_embed.num_patches + self.num_tokens, embed_dim))
        self.pos_drop = nn.Dropout(p=drop_rate)
        dpr = [x.item() for x in torch.linspace(0, drop_path_rate, depth)]      # stochastic depth decay rule
        self.blocks = nn.Sequential(*[
            TTBlock(dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, drop=drop_rate,
                    attn_drop=attn_drop_rate, drop_path=dpr[i], norm_layer=norm_layer, act_layer=act_layer,
                    linear=linear, block_id=i, hp_dict=hp_dict, dense_dict=dense_dict)
            for i in range(depth)])
        self.norm = norm_layer(embed_dim)
        self.pre_logits = nn.Identity()
        self.head = nn.Linear(embed_dim, num_classes) if num_classes > 0 else nn.Identity()
        self.head_dist = None
        if distilled:
            self.head_dist = nn.Linear(embed_dim, num_classes) if num_classes > 0 else nn.Identity()
        _trunc_normal_(self.pos_embed)
        _trunc_normal_(self.cls_token)
        if distilled:
            _trunc_normal_(self.dist_token)
        for m in (self.head, self.head_dist):
            if isinstance(m, nn.Linear):
                _trunc_normal_(m.weight)
                nn.init.zeros_(m.bias)

    def set_route(self, route):
        for blk in self.blocks:
            blk.set_route(route)
        return self

    def forward_features(self, x):
        x = self.patch_embed(x)
        tokens = [self.cls_token.expand(x.shape[0], -1, -1)]
        if self.dist_token is not None:
            tokens.append(self.dist_token.expand(x.shape[0], -1, -1))
        x = self.pos_drop(torch.cat(tokens + [x], dim=1) + self.pos_embed)
        normed = None
        last = len(self.blocks) - 1
        for i, blk in enumerate(self.blocks):
            x, normed = blk(x, normed, self.blocks[i + 1].norm1 if i < last else self.norm)
        if normed is None:
            normed = self.norm(x)
        if self.dist_token is None:
            return self.pre_logits(normed[:, 0])
        return normed[:, 0], normed[:, 1]

    def forward(self, x):
        x = self.forward_features(x)
        if self.head_dist is None:
            return self.head(x)
        x, x_dist = self.head(x[0]), self.head_dist(x[1])
        if self.training and not torch.jit.is_scripting():
            return x, x_dist
        return (x + x_dist) / 2


def _tt_vit(patch_size=16, embed_dim=384, depth=12, num_heads=6, mlp_ratio=4, qkv_bias=True, linear=TTLinearM,
            hp_dict=None, dense_dict=None, **kwargs):
    model = TTVisionTransformer(patch_size=patch_size, embed_dim=embed_dim, depth=depth, num_heads=num_heads,
                                mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, linear=linear, hp_dict=hp_dict,
                                dense_dict=dense_dict, **kwargs)
    if dense_dict is not None:                  # the dense parts take the dense model's values (vit_tt.py:139-144)
        state = model.state_dict()
        for key in state:
            if key in dense_dict:
                state[key] = dense_dict[key]
        model.load_state_dict(state)
    return model


def _factory(name, linear, **arch):
    def create(hp_dict, pretrained=False, decompose=False, path=None, dense_dict=None, **kwargs):
        return create_model(name, partial(_tt_vit, linear=linear, **{**arch, **kwargs}), hp_dict, decompose, pretrained,
                            path, dense_dict)
    create.__name__ = create.__qualname__ = name
    create.__doc__ = (f"vit_tt.py: {name}(hp_dict, pretrained=False, decompose=False, path=None, dense_dict=None, **kwargs).  "
                      "decompose=True factorises the dense state dict given as dense_dict= (or saved at the local `path`); "
                      "pretrained=True loads a compressed state dict from the local `path`.")
    return create


_ARCH = {
    "vit_small_patch16_224": dict(patch_size=16, embed_dim=384, depth=12, num_heads=6),
    "deit_tiny_patch16_224": dict(patch_size=16, embed_dim=192, depth=12, num_heads=3, mlp_ratio=4, qkv_bias=True),
    "deit_small_patch16_224": dict(patch_size=16, embed_dim=384, depth=12, num_heads=6, mlp_ratio=4, qkv_bias=True),
}
_LINEAR = {"ttm": TTLinearM, "ttr": TTLinearR, "tkm": TKLinearM, "tkr": TKLinearR}
FACTORIES = tuple(f"{kind}_{arch}" for kind in _LINEAR for arch in _ARCH)
for _kind, _lin in _LINEAR.items():
    for _arch, _kw in _ARCH.items():
        globals()[f"{_kind}_{_arch}"] = _factory(f"{_kind}_{_arch}", _lin, **_kw)
del _kind, _lin, _arch, _kw

__all__ = ["DropPath", "PatchEmbed", "TTAttention", "TTMlp", "TTBlock", "TTVisionTransformer", "FACTORIES"] + list(FACTORIES)
