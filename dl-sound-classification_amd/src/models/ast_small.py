"""ASTViTSmall — drop-in for the reference ``src.models.ast_small.ASTViTSmall`` (model=ast_small): a 12-block,
384-wide, 6-head ViT on log-mel patches that trains from scratch (no DeiT checkpoint).

Same Hydra target, constructor signature and defaults, same module tree built in the same order from the real
torch containers -- ``patch_embed.proj`` (Conv2d), ``cls_token``, ``pos_embed``, ``blocks.<i>.{norm1, attn
(nn.MultiheadAttention(dropout=0.1, batch_first=True)), norm2, mlp (Linear, GELU, Dropout(0.1), Linear,
Dropout(0.1))}``, ``norm``, ``head`` -- so ``state_dict()`` keys and shapes and the default initialisation under a
given ``torch.manual_seed`` are the reference's by construction.  Same forward contract: (B, F, T) or (B, 1, F, T)
log-mel -> (B, classes) sigmoid probabilities of the CLS token; ``pos_embed[:, :N]`` is the table's first N rows.

The containers only hold parameters: the math runs on the HIP kernels through ``ast_hip.ASTFunction`` (one
autograd node), which reads from this module LayerNorm eps 1e-5 and, in training mode, the three dropout rates:
on the attention probabilities (inside the attention kernels), after GELU and after fc2.  ``dropout_seeds`` =
a (depth, 3) integer table pins the mask seeds (tests); None draws fresh seeds per call.  trainer.precision
fp8-mixed runs these models in bf16.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from ..miaudio import lib as L
from .ast_hip import ASTFunction


class PatchEmbed(nn.Module):
    def __init__(self, in_chans=1, emb_dim=384, patch_size=16, stride=10):
        super().__init__()
        self.proj = nn.Conv2d(in_chans, emb_dim, kernel_size=patch_size, stride=stride)


class TransformerEncoderBlock(nn.Module):
    """Parameter container of one pre-LN block (the math lives in ast_hip)."""

    def __init__(self, emb_dim=384, num_heads=6, mlp_ratio=4.0, dropout=0.1):
        super().__init__()
        self.norm1 = nn.LayerNorm(emb_dim)
        self.attn = nn.MultiheadAttention(emb_dim, num_heads, dropout=dropout, batch_first=True)
        self.norm2 = nn.LayerNorm(emb_dim)
        self.mlp = nn.Sequential(
            nn.Linear(emb_dim, int(mlp_ratio * emb_dim)),
            nn.GELU(),
            nn.Dropout(dropout),
            nn.Linear(int(mlp_ratio * emb_dim), emb_dim),
            nn.Dropout(dropout),
        )


class SmallAST(nn.Module):
    """What ASTViTSmall and ASTMiniViT share; they differ in their defaults only."""

    def __init__(self, sample_rate, patch_size, patch_stride, overlap, num_classes, emb_dim, depth, num_heads, f_dim):
        super().__init__()
        if emb_dim != 64 * num_heads:
            raise ValueError(f"the attention kernels are head-dim 64: emb_dim {emb_dim} needs {emb_dim // 64} heads")
        self.f_dim = f_dim
        self.num_classes = num_classes
        self.emb_dim = emb_dim
        self.num_heads = num_heads
        self.patch_size, self.patch_stride = patch_size, patch_stride
        self.t_dim = int((sample_rate * 10) / 160) + 1  # 10 s clips at hop 160
        self.patch_embed = PatchEmbed(in_chans=1, emb_dim=emb_dim, patch_size=patch_size, stride=patch_stride)
        self.grid_size = ((self.f_dim - patch_size) // (patch_size - overlap) + 1,
                          (self.t_dim - patch_size) // (patch_size - overlap) + 1)
        num_patches = self.grid_size[0] * self.grid_size[1]
        self.cls_token = nn.Parameter(torch.zeros(1, 1, emb_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, 1 + num_patches, emb_dim))
        nn.init.trunc_normal_(self.pos_embed, std=0.02)
        self.blocks = nn.Sequential(*[TransformerEncoderBlock(emb_dim=emb_dim, num_heads=num_heads)
                                      for _ in range(depth)])
        self.norm = nn.LayerNorm(emb_dim)
        self.head = nn.Linear(emb_dim, num_classes)
        self.compute_dtype = None
        self.dropout_seeds = None

    # what ast_hip reads
    @property
    def ln_eps(self) -> float:
        return self.norm.eps

    @property
    def attn_drop(self) -> float:
        return float(self.blocks[0].attn.dropout) if len(self.blocks) else 0.0

    @property
    def act_drop(self) -> float:
        return float(self.blocks[0].mlp[2].p) if len(self.blocks) else 0.0

    @property
    def out_drop(self) -> float:
        return float(self.blocks[0].mlp[4].p) if len(self.blocks) else 0.0

    def _compute_code(self) -> int:
        cd = self.compute_dtype
        if cd is None:
            if torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") == torch.bfloat16:
                return L.BF16
            return L.F32
        # fp8-mixed: these models run bf16 (no MX path under dropout; EnvNet-v2 does the same)
        return {"bf16": L.BF16, "bfloat16": L.BF16, "f32": L.F32, "fp32": L.F32, "32": L.F32, "fp8": L.BF16}[str(cd)]

    def param_list(self):
        ps = [self.patch_embed.proj.weight, self.patch_embed.proj.bias, self.cls_token, self.pos_embed]
        for blk in self.blocks:
            ps += [blk.norm1.weight, blk.norm1.bias, blk.attn.in_proj_weight, blk.attn.in_proj_bias,
                   blk.attn.out_proj.weight, blk.attn.out_proj.bias, blk.norm2.weight, blk.norm2.bias,
                   blk.mlp[0].weight, blk.mlp[0].bias, blk.mlp[3].weight, blk.mlp[3].bias]
        ps += [self.norm.weight, self.norm.bias, self.head.weight, self.head.bias]
        return ps

    def forward(self, x):
        if x.dim() == 4:
            x = x[:, 0]
        params = self.param_list()
        grad = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params))
        with torch.autocast("cuda", enabled=False):
            return ASTFunction.apply(self, x, self._compute_code(), grad, *params)


class ASTViTSmall(SmallAST):
    def __init__(self, sample_rate=44100, patch_size=16, patch_stride=10, overlap=6, num_classes=50, emb_dim=384,
                 depth=12, num_heads=6, f_dim=128):
        super().__init__(sample_rate, patch_size, patch_stride, overlap, num_classes, emb_dim, depth, num_heads, f_dim)
