"""ASTMiniViT — drop-in for the reference ``src.models.ast_mini.ASTMiniViT`` (model=ast_mini): the 6-block,
192-wide, 3-head member of the small-AST family.  Everything but the defaults is ``ast_small.SmallAST``: same
module tree and state-dict names as the reference, the math on the HIP kernels through ``ast_hip.ASTFunction``."""
from __future__ import annotations

from .ast_small import PatchEmbed, SmallAST, TransformerEncoderBlock  # noqa: F401  (the reference module's names)


class ASTMiniViT(SmallAST):
    def __init__(self, sample_rate=44100, patch_size=16, patch_stride=10, overlap=6, num_classes=50, emb_dim=192,
                 depth=6, num_heads=3, f_dim=128):
        super().__init__(sample_rate, patch_size, patch_stride, overlap, num_classes, emb_dim, depth, num_heads, f_dim)
