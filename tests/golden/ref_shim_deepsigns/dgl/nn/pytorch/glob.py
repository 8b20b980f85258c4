"""dgl.nn.pytorch.glob.SetTransformerEncoder (block type 'sab'), restated from DGL's published definition: the sets of a batch are
padded to the largest graph, attended densely under a length mask, and unpadded again."""
import math

import torch
import torch.nn as nn


class MultiHeadAttention(nn.Module):
    def __init__(self, d_model, num_heads, d_head, d_ff, dropouth=0., dropouta=0.):
        super().__init__()
        self.d_model, self.num_heads, self.d_head, self.d_ff = d_model, num_heads, d_head, d_ff
        self.proj_q = nn.Linear(d_model, num_heads * d_head, bias=False)
        self.proj_k = nn.Linear(d_model, num_heads * d_head, bias=False)
        self.proj_v = nn.Linear(d_model, num_heads * d_head, bias=False)
        self.proj_o = nn.Linear(num_heads * d_head, d_model, bias=False)
        self.ffn = nn.Sequential(nn.Linear(d_model, d_ff), nn.ReLU(), nn.Dropout(dropouth), nn.Linear(d_ff, d_model))
        self.droph = nn.Dropout(dropouth)
        self.dropa = nn.Dropout(dropouta)
        self.norm_in = nn.LayerNorm(d_model)
        self.norm_inter = nn.LayerNorm(d_model)
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)

    def forward(self, x, mem, lengths_x, lengths_mem):
        batch, max_x, max_mem = len(lengths_x), max(lengths_x), max(lengths_mem)
        H, dh = self.num_heads, self.d_head

        def pad(t, lengths, width):
            out = t.new_zeros(batch, width, t.shape[-1])
            o = 0
            for b, n in enumerate(lengths):
                out[b, :n] = t[o:o + n]
                o += n
            return out

        q = pad(self.proj_q(x), lengths_x, max_x).view(batch, max_x, H, dh)
        k = pad(self.proj_k(mem), lengths_mem, max_mem).view(batch, max_mem, H, dh)
        v = pad(self.proj_v(mem), lengths_mem, max_mem).view(batch, max_mem, H, dh)
        e = torch.einsum("bxhd,byhd->bhxy", q, k) / math.sqrt(dh)
        lx, lm = torch.as_tensor(lengths_x), torch.as_tensor(lengths_mem)
        mask = ((torch.arange(max_x)[None, :] < lx[:, None])[:, None, :, None] &
                (torch.arange(max_mem)[None, :] < lm[:, None])[:, None, None, :])
        e = e.masked_fill(~mask, float("-inf"))
        alpha = torch.softmax(e, dim=-1).masked_fill(~mask, 0.)
        out = torch.einsum("bhxy,byhd->bxhd", alpha, v)
        out = self.proj_o(out.contiguous().view(batch, max_x, H * dh))
        out = torch.cat([out[b, :n] for b, n in enumerate(lengths_x)], dim=0)
        x = self.norm_in(x + out)
        x = self.norm_inter(x + self.ffn(x))
        return x


class SetAttentionBlock(nn.Module):
    def __init__(self, d_model, num_heads, d_head, d_ff, dropouth=0., dropouta=0.):
        super().__init__()
        self.mha = MultiHeadAttention(d_model, num_heads, d_head, d_ff, dropouth=dropouth, dropouta=dropouta)

    def forward(self, feat, lengths):
        return self.mha(feat, feat, lengths, lengths)


class SetTransformerEncoder(nn.Module):
    def __init__(self, d_model, n_heads, d_head, d_ff, n_layers=1, block_type="sab", m=None, dropouth=0., dropouta=0.):
        super().__init__()
        assert block_type == "sab"
        self.layers = nn.ModuleList([SetAttentionBlock(d_model, n_heads, d_head, d_ff, dropouth=dropouth, dropouta=dropouta)
                                     for _ in range(n_layers)])

    def forward(self, graph, feat):
        lengths = [int(n) for n in graph.batch_num_nodes()]
        for layer in self.layers:
            feat = layer(feat, lengths)
        return feat
