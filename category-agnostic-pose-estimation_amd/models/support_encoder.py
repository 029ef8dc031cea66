"""The reference's default support encoder (reference `models/support_encoder.py:8-229`, built by `CAPEModel` unless
`--use_geometric_encoder` is passed) on MI355X kernels: coordinate MLP -> [coord_emb | degree-scaled edge embedding] ->
coord_edge_proj -> dropout(x + sine PE) -> 3 post-norm transformer encoder layers with key-padding mask -> LayerNorm.

Same constructor, child names and `state_dict` as the reference (`pos_embedding.pe` is a persistent (1, 5000, C) buffer).
Semantics kept from the reference:
  * the mask: `support_mask` arrives un-inverted from CAPEModel and `~support_mask` is the key-padding mask, so attention sees
    only the keypoints the sampler marks True; a graph with no such keypoint has every key masked.  There is no all-masked guard:
    such rows get zero attention (torch's result with grad enabled), `mask_mode=3` of the attention kernels;
  * eval under no_grad takes nn.TransformerEncoder's nested-tensor path when the padding mask is left-aligned over the batch:
    padded rows leave the layer stack as 0 and the final norm turns them into `norm.bias`.  When EVERY graph of such a batch is
    fully masked the reference raises (to_padded_tensor of an all-empty nested tensor); here the rows come out as `norm.bias` --
    the one deliberate deviation;
  * edge rules of `_build_adjacency_matrix` (index s-1 if s > 0, kept if inside [0, N), symmetric, duplicates once, visibility
    ignored), `edge_info = edge_embedding[deg > 0] * clamp(deg, 1) / 10`; that branch runs only for a non-empty skeleton list.
`SupportGraphAggregator` is not used by the reference's model and is not provided."""
import math

import torch
import torch.nn as nn

from ..hip import functional as HF
from ..hip import ops
from .graph_utils import DeviceSkeleton, _edge_tables


class PositionalEncoding1D(nn.Module):
    """Sinusoidal PE over the keypoint index + dropout (reference support_encoder.py:134-159)."""

    def __init__(self, d_model, dropout=0.1, max_len=5000):
        super().__init__()
        self.dropout = nn.Dropout(p=dropout)
        pe = torch.zeros(max_len, d_model)
        position = torch.arange(0, max_len, dtype=torch.float).unsqueeze(1)
        div_term = torch.exp(torch.arange(0, d_model, 2).float() * (-math.log(10000.0) / d_model))
        pe[:, 0::2] = torch.sin(position * div_term)
        pe[:, 1::2] = torch.cos(position * div_term)
        self.register_buffer("pe", pe.unsqueeze(0))
        self._stream = ops.new_stream_id()

    def forward(self, x):
        if x.shape[1] > self.pe.shape[1]:
            raise RuntimeError(f"{x.shape[1]} keypoints exceed PositionalEncoding1D.max_len={self.pe.shape[1]}")
        p = self.dropout.p if self.training else 0.0
        return HF.pe_dropout(x, self.pe[0], p, self._stream)


class SupportPoseGraphEncoder(nn.Module):
    def __init__(self, hidden_dim=256, nheads=8, num_encoder_layers=3, dim_feedforward=1024, dropout=0.1, max_keypoints=50):
        super().__init__()
        if hidden_dim != 256 or nheads != 8:
            raise ValueError("MI355X kernels: hidden_dim=256, 8 heads (reference defaults)")
        self.hidden_dim = hidden_dim
        self.nheads = nheads
        self.max_keypoints = max_keypoints
        self.coord_embedding = nn.Sequential(nn.Linear(2, hidden_dim), nn.ReLU(), nn.Linear(hidden_dim, hidden_dim))
        self.edge_embedding = nn.Embedding(num_embeddings=2, embedding_dim=hidden_dim)
        self.coord_edge_proj = nn.Linear(hidden_dim * 2, hidden_dim)
        self.pos_embedding = PositionalEncoding1D(hidden_dim, dropout=dropout)
        layer = nn.TransformerEncoderLayer(d_model=hidden_dim, nhead=nheads, dim_feedforward=dim_feedforward, dropout=dropout,
                                           activation="relu", batch_first=True)
        self.transformer_encoder = nn.TransformerEncoder(layer, num_layers=num_encoder_layers)
        self.norm = nn.LayerNorm(hidden_dim)
        self._reset_parameters()
        self.dropout_p = dropout
        self._streams = [[ops.new_stream_id() for _ in range(4)] for _ in range(num_encoder_layers)]

    def _reset_parameters(self):
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)

    def _edge_tables(self, skeleton_edges, dev):
        if isinstance(skeleton_edges, DeviceSkeleton):
            return skeleton_edges.edges.contiguous(), skeleton_edges.start
        flat, start = [], [0]
        for edges in skeleton_edges:
            for e in (edges if edges is not None else []):
                if len(e) == 2:                          # (support_encoder.py:109: other entries are skipped)
                    flat.append((int(e[0]), int(e[1])))
            start.append(len(flat))
        return _edge_tables(flat, start, dev)[:2]

    def embed(self, support_coords, skeleton_edges=None):
        """coord_embedding (+ edge info + coord_edge_proj) + pos_embedding: the encoder input (B, N, C)."""
        B, N, _ = support_coords.shape
        m0, m2 = self.coord_embedding[0], self.coord_embedding[2]
        h = HF.legacy_coord_embed(support_coords, m0.weight, m0.bias)
        if skeleton_edges is not None and len(skeleton_edges) > 0:
            if len(skeleton_edges) != B:
                raise ValueError(f"skeleton_edges holds {len(skeleton_edges)} graphs for a batch of {B}")
            edges, start = self._edge_tables(skeleton_edges, support_coords.device)
            cat = HF.edge_cat(h, m2.weight, m2.bias, self.edge_embedding.weight, edges, start)
            x = HF.linear(cat, self.coord_edge_proj.weight, self.coord_edge_proj.bias)
        else:
            x = HF.linear(h, m2.weight, m2.bias)
        return self.pos_embedding(x)

    def forward(self, support_coords, support_mask=None, skeleton_edges=None):
        B, N, _ = support_coords.shape
        x = self.embed(support_coords, skeleton_edges)
        kpm, mode = None, 0
        if support_mask is not None:
            kpm = ops.as_u8(~support_mask.bool())         # src_key_padding_mask = ~support_mask (support_encoder.py:85)
            mode = 3
        # nn.TransformerEncoder's nested-tensor path (eval, no grad, padding mask left-aligned over the batch): padded rows leave
        # the stack as zeros.  A host decision, taken only outside autograd, where the reference takes it too
        fast = False
        if kpm is not None and (not self.training) and (not torch.is_grad_enabled()):
            valid = support_mask.bool().to(torch.int8)
            fast = bool(((valid[:, 1:] - valid[:, :-1]) <= 0).all())
        p = self.dropout_p if self.training else 0.0
        for li, layer in enumerate(self.transformer_encoder.layers):
            sa, st = layer.self_attn, self._streams[li]
            x_a, x_r = HF.fanout(x, 2)
            a = HF.mha(x_a, x_a, x_a, sa.in_proj_weight, sa.in_proj_bias, sa.out_proj.weight, sa.out_proj.bias, self.nheads,
                       mask_mode=mode, kpm_u8=kpm, dropout_p=p, rng_stream=st[0])
            x = HF.add_layernorm(x_r, a, layer.norm1.weight, layer.norm1.bias, dropout_p=p, rng_stream=st[1])
            x_f, x_r = HF.fanout(x, 2)
            hdn = HF.ffn(x_f, layer.linear1.weight, layer.linear1.bias, layer.linear2.weight, layer.linear2.bias, dropout_p=p,
                         rng_stream=st[2])
            x = HF.add_layernorm(x_r, hdn, layer.norm2.weight, layer.norm2.bias, dropout_p=p, rng_stream=st[3])
        if fast:
            x = HF.zero_rows(x, kpm.reshape(-1))
        # the final LayerNorm is its own launch of the LayerNorm kernel (fusing it into the last add_layernorm
        # saves one ~2 us launch of a 544 x 256 row pass)
        return HF.add_layernorm(x, None, self.norm.weight, self.norm.bias)

    def __repr__(self):
        return f"{self.__class__.__name__}(hidden_dim={self.hidden_dim}, nheads={self.nheads}, edge_info=degree, sequence_pe=SinePE1D)"


def build_support_encoder(args):
    return SupportPoseGraphEncoder(hidden_dim=getattr(args, "hidden_dim", 256), nheads=getattr(args, "nheads", 8),
                                   num_encoder_layers=getattr(args, "support_encoder_layers", 3),
                                   dim_feedforward=getattr(args, "dim_feedforward", 1024), dropout=getattr(args, "dropout", 0.1))
