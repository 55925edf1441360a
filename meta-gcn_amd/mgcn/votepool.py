"""src/gcn_meta/models/gpool_hard_attention.py on the engine: graph pooling by
"voting" -- hard attention in the out direction, so that every node sends its
feature to one neighbour, and the graph is pruned to the nodes that received
a vote -- with the same names, constructor arguments, forward signatures,
return tuples and state_dict keys.

``x @ W`` runs on :func:`mgcn.ops.linear`, the message passing on
:func:`mgcn.ops.hard_attention_aggregate` (Gumbel-softmax in training, argmax
+ one-row gather in eval), the residual and read-out Linears are
:class:`mgcn.models.Linear`, the segment argmax of :func:`get_edge_select` is
:func:`mgcn.pool.scatter_max_arg`; the remaining index bookkeeping is torch on
the device.

Three defects of the reference are not mirrored:
 1. get_edge_select built its mask on the CPU (:105) and so failed on a GPU;
    here the mask lives on alpha's device.
 2. prune(relabel=True) returned ``end - kept_below_end`` as the new slice
    ends (:150-153); here they are the kept counts below each boundary.
 3. SATOutLayer's multi-graph branch filled the *valid* rows with -inf
    (:344-347); here the padded and zero rows are filled, and a graph with no
    row left yields proj(0), as the single-graph branch does.
Everything else is mirrored as is, including the ``x.sum(dim=1) > 1e-20`` row
filter, argmax -1 selecting the last edge in get_edge_select's training
branch, and prune zeroing the rows it does not keep.
"""
from __future__ import annotations

import torch
import torch.nn as nn
from torch.nn import Parameter
from torch.nn.utils.rnn import pad_sequence

from .graph import adopt_derived, plan_for
from .models import Linear, _edge_rng, activation, glorot, zeros
from .ops import DeviceDropout, DeviceGumbel, draw_edge_seed, hard_attention_aggregate, linear
from .pool import scatter_max_arg


def gumbel_samples(base):
    """gpool_hard_attention.py:13-21: iid Gumbel(0, 1) samples with the size,
    dtype and device of ``base``.  VotePoolLayer.forward calls it through this
    module global, once, with a float32 [E, nheads] tensor, and reads the
    result in COO edge order (tests replace the global to replay noise)."""
    noise = torch.rand(base.size()).to(base)
    eps = 1e-20
    noise.add_(eps).log_().neg_()
    noise.add_(eps).log_().neg_()
    return noise


def subgraph(subset, edge_index, edge_attr=None, relabel_nodes=False, num_nodes=None):
    """gpool_hard_attention.py:25-71 (torch_geometric.utils.subgraph with the
    masks on edge_index's device): the subgraph induced by ``subset`` (node
    ids, or a bool mask), optionally relabelled to consecutive ids."""
    return _subgraph(subset, edge_index, edge_attr, relabel_nodes, num_nodes)[:2]


def _subgraph(subset, edge_index, edge_attr=None, relabel_nodes=False, num_nodes=None):
    """:func:`subgraph`, returning the bool [E] mask of the kept edges as well."""
    device = edge_index.device
    if isinstance(subset, (list, tuple)):
        subset = torch.tensor(subset, dtype=torch.long, device=device)
    if subset.dtype == torch.bool or subset.dtype == torch.uint8:
        n_mask = subset.to(device=device, dtype=torch.bool)
        if relabel_nodes:
            n_idx = torch.zeros(n_mask.size(0), dtype=torch.long, device=device)
            n_idx[n_mask] = torch.arange(int(n_mask.sum().item()), device=device)
    else:
        if num_nodes is None:  # PyG 1.3 maybe_num_nodes
            num_nodes = int(edge_index.max()) + 1 if edge_index.numel() else 0
        n_mask = torch.zeros(num_nodes, dtype=torch.bool, device=device)
        n_mask[subset] = True
        if relabel_nodes:
            n_idx = torch.zeros(num_nodes, dtype=torch.long, device=device)
            n_idx[subset] = torch.arange(subset.size(0), device=device)
    mask = n_mask[edge_index[0]] & n_mask[edge_index[1]]
    edge_index = edge_index[:, mask]
    edge_attr = edge_attr[mask] if edge_attr is not None else None
    if relabel_nodes:
        edge_index = n_idx[edge_index]
    return edge_index, edge_attr, mask


def get_edge_select(x, edge_index, alpha, training=True, p_keep=None):
    """gpool_hard_attention.py:74-122: the bool [E] mask of the edges the
    pruning keeps.  Training: per source node and head the edge with the
    largest ``alpha`` (an argmax of -1 -- a node without out-edge -- selects
    the last edge, as the reference's indexing does); with ``p_keep`` (alpha
    after the softmax) every edge with some alpha >= p_keep, plus all edges of
    the nodes where some head's maximum stays below p_keep.  Eval: the edges
    with a non-zero one-hot entry.  ``x`` only supplies the node count."""
    if training:
        out, argmax = scatter_max_arg(alpha, edge_index[0], x.size(0), fill_value=-1e16)
        if p_keep is None:
            edge_select = torch.zeros(alpha.size(0), dtype=torch.bool, device=alpha.device)
            edge_select[argmax.view(-1)] = True
        else:
            node_keep = (out < p_keep).sum(dim=1) > 0
            edge_keep = node_keep[edge_index[0]]
            edge_select = ((alpha >= p_keep).sum(dim=1) > 0) | edge_keep
    else:
        edge_select = alpha.sum(dim=1) > 0
    return edge_select


def prune(x, edge_index, edge_select, relabel=False, batch_slices_x=None):
    """gpool_hard_attention.py:125-160: keep the nodes that a selected edge
    points to.  ``relabel=False`` zeroes the other rows of ``x`` (in place)
    and keeps ids and slices; ``relabel=True`` drops them, renumbers the edges
    and returns, for every graph boundary, the number of kept nodes below it.
    Returns (x, edge_index, nodes (sorted), batch_slices_x)."""
    nodes = edge_index[1, edge_select].unique()
    parent, n_parent = edge_index, x.size(0)
    if relabel:
        assert batch_slices_x is not None
        edge_index, _, kept = _subgraph(nodes, edge_index, relabel_nodes=True,
                                        num_nodes=x.size(0))
        x = x[nodes, :]
        batch_slices_x_pruned = [0]
        for end in batch_slices_x[1:]:
            batch_slices_x_pruned.append(int((nodes < end).sum().item()))
    else:
        edge_index, _, kept = _subgraph(nodes, edge_index, relabel_nodes=False,
                                        num_nodes=x.size(0))
        nodes_prune_mask = x.new_ones(x.size(0), dtype=torch.bool)
        nodes_prune_mask[nodes] = False
        x[nodes_prune_mask, :] = 0
        batch_slices_x_pruned = batch_slices_x
    # the next layer's plan: derived from this graph's (when it has one) rather
    # than rebuilt from the new edge list (graph.set_derived_plans)
    adopt_derived(parent, n_parent, kept, edge_index, x.size(0), nodes if relabel else None)
    return x, edge_index, nodes, batch_slices_x_pruned


class VotePoolLayer(nn.Module):
    """gpool_hard_attention.py:163-314: one pooling layer.  Hard attention
    with att_dir 'out' (every node chooses where to send its feature),
    aggregation at the targets, then pruning by :func:`get_edge_select` /
    :func:`prune`.  ``aggr``: 'add' is the kernel's sum, 'mean' that sum
    divided by max(in-degree, 1); 'max' is not implemented.
    ``edge_rng='device'`` (default 'torch', this module's ``gumbel_samples``):
    noise and dropout mask generated on the device, as for
    :class:`mgcn.models.NodeModelHardAttention`."""

    def __init__(self, in_channels, out_channels, nheads=1, att_act='none', att_dropout=0,
                 att_combine='cat', att_dir='out', bias=False, aggr='add', temperature=0.1,
                 sample=False, p_keep=None, relabel=False, edge_rng='torch', **kwargs):
        assert att_act in ['none', 'lrelu', 'relu']
        assert att_combine in ['cat', 'add', 'mean']
        assert att_dir == 'out'
        if aggr == 'max':
            raise NotImplementedError(
                "VotePoolLayer: aggr='max' is not implemented on the hard-attention kernels "
                "(use 'add' or 'mean')")
        assert aggr in ['add', 'mean']
        super().__init__()
        self.edge_rng = _edge_rng(edge_rng)
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.aggr = aggr
        self.p_keep = p_keep
        self.relabel = relabel
        self.nheads = nheads
        if att_combine == 'cat':
            self.out_channels_1head = out_channels // nheads
            assert self.out_channels_1head * nheads == out_channels, \
                'out_channels should be divisible by nheads'
        else:
            self.out_channels_1head = out_channels
        self.att_combine = att_combine
        self.att_dir = att_dir
        self.att_act_name = att_act
        self.temperature = temperature
        self.sample = sample
        self.weight = Parameter(torch.Tensor(in_channels, self.out_channels_1head * nheads))
        self.att_weight = Parameter(torch.Tensor(1, nheads, 2 * self.out_channels_1head))
        self.att_act = activation(att_act)
        self.att_dropout = nn.Dropout(p=att_dropout)
        if bias:
            self.bias = Parameter(torch.Tensor(out_channels))
        else:
            self.register_parameter('bias', None)
        self.reset_parameters()

    def reset_parameters(self):
        glorot(self.weight)
        glorot(self.att_weight)
        zeros(self.bias)

    def forward(self, x, edge_index, batch_slices_x, attn_store=None):
        plan = plan_for(edge_index, x.size(0))
        hp = linear(x, self.weight)
        noise = mask = None
        device_rng = self.edge_rng == 'device'
        if (self.training or self.sample) and device_rng:
            noise = DeviceGumbel(*draw_edge_seed())
        elif self.training or self.sample:
            noise = gumbel_samples(torch.empty(plan.nnz, self.nheads, dtype=torch.float32,
                                               device=hp.device))
        if self.training and self.att_dropout.p > 0 and device_rng:
            mask = DeviceDropout(self.att_dropout.p, *draw_edge_seed())
        elif self.training and self.att_dropout.p > 0:
            mask = nn.functional.dropout(
                torch.ones(plan.nnz, self.nheads, dtype=torch.float32, device=hp.device),
                p=self.att_dropout.p, training=True)
        y, alpha = hard_attention_aggregate(hp, self.att_weight, plan, self.nheads,
                                            self.att_act_name, self.att_dir, self.temperature,
                                            training=self.training, noise=noise, edge_mask=mask)
        if self.aggr == 'mean':
            y = y / plan.in_cnt.view(-1, 1)
        if self.att_combine == 'add':
            y = y.view(-1, self.nheads, self.out_channels_1head).sum(dim=1)
        elif self.att_combine == 'mean':
            y = y.view(-1, self.nheads, self.out_channels_1head).mean(dim=1)
        if self.bias is not None:
            y = y + self.bias
        if attn_store is not None:
            attn_store.append(alpha)
        with torch.no_grad():
            edge_select = get_edge_select(y, edge_index, alpha, training=self.training,
                                          p_keep=self.p_keep)
        if not self.relabel:
            y = y.clone()  # prune writes zeros in place; the op's output stays intact
        return prune(y, edge_index, edge_select, relabel=self.relabel,
                     batch_slices_x=batch_slices_x)

    @property
    def num_parameters(self):
        if not hasattr(self, 'num_para'):
            self.num_para = sum([p.nelement() for p in self.parameters()])
        return self.num_para

    def __repr__(self):
        return ('{} (in_channels: {}, out_channels: {}, nheads: {}, att_activation: {},'
                'att_dropout: {}, att_combine: {}, att_dir: {}, temperature: {}, sample: {}, '
                'pruning_p: {}, pruning_relabel: {} | number of parameters: {})').format(
                    self.__class__.__name__, self.in_channels, self.out_channels, self.nheads,
                    self.att_act, self.att_dropout.p, self.att_combine, self.att_dir,
                    self.temperature, self.sample, self.p_keep, self.relabel,
                    self.num_parameters)


class SATOutLayer(nn.Module):
    """gpool_hard_attention.py:317-351: the read-out.  A softmax self-attention
    over the rows of a graph whose sum exceeds 1e-20 (the pruned rows are
    zero), then a projection to the classes.  Several graphs are padded to one
    [B, max nodes, C] batch; the padded and the zero rows are masked out, and a
    graph with no row left gives proj(0), as the single-graph branch does."""

    def __init__(self, channels, num_classes):
        super().__init__()
        self.channels = channels
        self.num_classes = num_classes
        self.self_attention = Linear(channels, 1, bias=True)
        self.proj = Linear(channels, num_classes, bias=True)

    def reset_parameters(self):
        self.self_attention.reset_parameters()
        self.proj.reset_parameters()

    def forward(self, x, batch_slices_x):
        if len(batch_slices_x) == 2:
            x = x[x.sum(dim=1) > 1e-20]
            scores = self.self_attention(x) if x.size(0) else x.new_zeros(0, 1)
            attn_weights = nn.functional.softmax(scores, dim=0)
            out = self.proj((x * attn_weights.view(-1, 1)).sum(dim=0, keepdim=True))
        else:
            x_batch = [x[i:j] for (i, j) in zip(batch_slices_x, batch_slices_x[1:])]
            x_batch = pad_sequence(x_batch, batch_first=True, padding_value=0)
            valid = x_batch.sum(dim=-1) > 1e-20  # [B, max nodes]
            B, M, C = x_batch.shape
            attn_scores = self.self_attention(x_batch.reshape(B * M, C)).view(B, M, 1)
            attn_scores = attn_scores.masked_fill(~valid.unsqueeze(2), float('-inf'))
            # a graph without a valid row: all -inf would give NaN; its rows are 0 anyway
            attn_scores = attn_scores.masked_fill(~valid.any(dim=1).view(-1, 1, 1), 0.0)
            # ... and its weights are dropped, so that no gradient reaches rows the
            # single-graph branch would have filtered out
            attn_weights = nn.functional.softmax(attn_scores, dim=1) * valid.unsqueeze(2)
            out = self.proj((x_batch * attn_weights).sum(dim=1))
        return out


class VotePoolModel(nn.Module):
    """gpool_hard_attention.py:354-425: VotePoolLayers with optional residual
    Linears and a non-linearity, then :class:`SATOutLayer`, for graph
    classification.  ``nheads`` may be an int or one value per layer; the other
    keyword arguments go to every layer."""

    def __init__(self, in_channels, enc_sizes, num_classes, non_linear='relu', residual=True,
                 dropout=0.0, **kwargs):
        super().__init__()
        self.in_channels = in_channels
        self.enc_sizes = [in_channels, *enc_sizes]
        self.num_layers = len(self.enc_sizes) - 1
        self.num_classes = num_classes
        self.residual = residual
        if 'nheads' in kwargs:
            if isinstance(kwargs['nheads'], int):
                self.nheads = [kwargs['nheads']] * self.num_layers
            elif isinstance(kwargs['nheads'], list):
                self.nheads = kwargs['nheads']
                assert len(self.nheads) == self.num_layers
            else:
                raise ValueError
            del kwargs['nheads']
        else:
            self.nheads = [1] * self.num_layers
        self.gpool_net = nn.ModuleList([
            VotePoolLayer(in_c, out_c, nheads=nh, **kwargs)
            for in_c, out_c, nh in zip(self.enc_sizes, self.enc_sizes[1:], self.nheads)])
        self.dropout = nn.Dropout(dropout)
        if residual:
            self.residual_net = nn.ModuleList([
                Linear(in_c, out_c, bias=True)
                for in_c, out_c in zip(self.enc_sizes, self.enc_sizes[1:])])
            self.num_residuals = len(self.residual_net)
        self.non_linear = activation(non_linear)
        self.out_net = SATOutLayer(enc_sizes[-1], num_classes)

    def reset_parameters(self):
        if self.residual:
            for net, rnet in zip(self.gpool_net, self.residual_net):
                net.reset_parameters()
                rnet.reset_parameters()
        else:
            for net in self.gpool_net:
                net.reset_parameters()
        self.out_net.reset_parameters()

    def forward(self, x, edge_index, batch_slices_x, remaining_nodes=None):
        for n, net in enumerate(self.gpool_net):
            xo, edge_index, nodes, batch_slices_x = net(x, edge_index, batch_slices_x)
            xo = self.dropout(xo)
            if self.residual:
                xr = self.residual_net[n](x)
                if net.relabel:
                    xr = xr[nodes]
                else:
                    keep = torch.zeros(xo.size(0), 1, dtype=xr.dtype, device=xr.device)
                    keep[nodes] = 1
                    xr = xr * keep
                x = self.non_linear(xo + xr)
            else:
                x = self.non_linear(xo)
            if remaining_nodes is not None:
                remaining_nodes.append(nodes)
        return self.out_net(x, batch_slices_x)


__all__ = ["gumbel_samples", "subgraph", "get_edge_select", "prune", "VotePoolLayer", "SATOutLayer",
           "VotePoolModel"]
