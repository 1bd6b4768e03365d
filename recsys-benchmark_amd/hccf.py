"""HCCF backbone with the propagation as fused leaky-residual SpMM HIP kernels.

Drop-in for src/models/hccf.py:8-80: same constructor, `forward(matrix) -> (user_emb, item_emb)` on the U x I
normalised matrix (`graph_utils.get_adj(..., normalize=True)`, `DeviceCFGraphDataset(adj_style="hccf")`),
`get_reg_loss`, attribute names and state_dict keys (`user_emb_table.weight`, `item_emb_table.weight`: the two
tables are plain nn.Embedding, as in the reference).
"""
import torch
from torch import nn

from . import _kernels, _lib
from .layers import SparseDropout
from .lightgcn import IGraphBaseCore


class HCCFModelCore(IGraphBaseCore):
    def __init__(self, num_user, num_item, num_layers=2, hidden_size=64, slope=0.5, p_dropout=0.5):
        super().__init__()
        self.user_emb_table = nn.Embedding(num_user, hidden_size)
        self.item_emb_table = nn.Embedding(num_item, hidden_size)
        self.activation = nn.LeakyReLU(slope)          # kept for the module tree; its slope is what the kernels apply
        self.num_layers = num_layers
        self._p_dropout = p_dropout
        self.sparse_dropout = SparseDropout(p_dropout) if p_dropout > 0 else nn.Identity()
        self._init_weight()

    def _init_weight(self):
        nn.init.xavier_uniform_(self.user_emb_table.weight)
        nn.init.xavier_uniform_(self.item_emb_table.weight)

    def get_emb_table(self, matrix):
        """matrix: sparse (num_user, num_item) normalised matrix -> (user_emb, item_emb).  In training with dropout one
        draw per layer serves both products of that layer (src/models/hccf.py:53-57); otherwise one matrix serves all."""
        users, items = self.user_emb_table.weight, self.item_emb_table.weight
        _lib.require_gpu(users, items, matrix)
        if self.training and self._p_dropout > 0:
            matrix = [self.sparse_dropout(matrix) for _ in range(self.num_layers)]
        else:
            matrix = self.sparse_dropout(matrix)
        return _kernels.hccf_propagate(matrix, users, items, self.num_layers, self.activation.negative_slope)

    def get_reg_loss(self, users, pos_items, neg_items) -> torch.Tensor:
        """(|e_u|^2 + |e_i+|^2 + |e_i-|^2) / (2 * batch) over the batch's rows of the two tables."""
        from .losses import reg_loss_rows

        return reg_loss_rows(self.user_emb_table.weight, self.item_emb_table.weight, users, pos_items, neg_items)

    def get_embs(self):
        return [("user", self.user_emb_table), ("item", self.item_emb_table)]
