"""gcn_meta module surface (src/gcn_meta/models/*) on the mgcn engine.

Same class names, constructor arguments, forward signatures, parameter names
and initialisation as the reference, so ``state_dict``s load in either
direction and the training scripts (src/run/train_botnet.py:190-294) run
unchanged after swapping the import:

  NodeModelBase / NodeModelAdditive  gcn_base_models.py:11-243
  EdgeGateProj / EdgeGateFree        gcn_base_models.py:322-396
  NodeModelGatedAdditive             NodeModelAdditive with an edge gate
  NodeModelAttention                 graph_attention.py:11-123
  GCNMultiKernel                     gcn_multi_kernel.py:9-114
  GCNLayer / GCNModel                gcn_model.py:8-197
  activation / Identity / scatter_   common.py:11-66

The aggregation (gather, degree normalisation, reduce, bias, ReLU) is one HIP
kernel per direction (:func:`mgcn.ops.aggregate`); the feature transform
``x @ W`` (gcn_base_models.py:201) runs on libmgcn's MFMA GEMMs through
:func:`mgcn.ops.linear` (bf16x6 arithmetic, fp32 accuracy), with a fused
backward (dW, dX, ReLU mask, bias column sums in one kernel); residual layers
fuse their skip projection into the same GEMM (:func:`mgcn.ops.residual_gcn_layer`).
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn
from torch.nn import Parameter
from torch.nn.utils.rnn import pad_sequence

from . import _lib as L
from . import ops as _ops
from .graph import plan_for
from .ops import (aggregate_plan, attention_aggregate, gcn_layer, gcn_stack, linear, linear_bias,  # noqa: F401
                  gate_aggregate, hard_attention_aggregate, multi_aggregate, multi_kernel_fusable,
                  multi_kernel_reason,
                  residual_gcn_layer, residual_layer_supported, residual_stack,  # noqa: F401
                  scatter_)
from .ops_noise import DeviceDropout, DeviceGumbel, draw_edge_seed


# --------------------------------------------------------------- inits (PyG)
def _wants_norm_grad(deg, edge_weight) -> bool:
    """A gradient is asked of deg / edge_weight (lists: the K kernels')."""
    if not torch.is_grad_enabled():
        return False
    ts = []
    for t in (deg, edge_weight):
        ts += list(t) if isinstance(t, (list, tuple)) else [t]
    return any(isinstance(t, torch.Tensor) and t.requires_grad for t in ts)


def glorot(tensor):
    """torch_geometric.nn.inits.glorot (used at gcn_base_models.py:193)."""
    if tensor is not None:
        stdv = math.sqrt(6.0 / (tensor.size(-2) + tensor.size(-1)))
        tensor.data.uniform_(-stdv, stdv)


def zeros(tensor):
    """torch_geometric.nn.inits.zeros (gcn_base_models.py:197)."""
    if tensor is not None:
        tensor.data.fill_(0)


class Linear(nn.Linear):
    """torch.nn.Linear with identical parameters/state_dict, whose products run
    on libmgcn (x W^T and dx on mgcn_gemm_nn, dW on the split-K mgcn_gemm_tn).
    Used for GCNModel's residual and final projections (gcn_model.py:64-73)."""

    def forward(self, input):
        return linear_bias(input, self.weight, self.bias)


# ------------------------------------------------------------- common.py
class Identity(nn.Module):
    """common.py:11-24"""

    def __init__(self, *args, **kwargs):
        super().__init__()

    def forward(self, input):
        return input


def activation(act, negative_slope=0.2):
    """common.py:27-34"""
    activations = nn.ModuleDict([
        ['lrelu', nn.LeakyReLU(negative_slope)],
        ['relu', nn.ReLU()],
        ['elu', nn.ELU()],
        ['none', Identity()],
    ])
    return activations[act]


# ------------------------------------------------------- gcn_base_models.py
class NodeModelBase(nn.Module):
    """gcn_base_models.py:11-160 (constructor checks and degnorm_const)."""

    def __init__(self, in_channels, out_channels, in_edgedim=None, deg_norm=None, edge_gate=None,
                 aggr='add', *args, **kwargs):
        assert deg_norm in [None, 'sm', 'rw']
        assert edge_gate in [None, 'proj', 'free']
        assert aggr in ['add', 'mean', 'max']
        super().__init__()
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.in_edgedim = in_edgedim
        self.deg_norm = deg_norm
        self.aggr = aggr
        if edge_gate is not None and not self._gated:
            # the plain class keeps its launch path; gates live in the subclass
            raise NotImplementedError(
                "edge_gate is not supported by NodeModelAdditive on the mgcn engine: use "
                "NodeModelGatedAdditive (GCNMultiKernel / GCNLayer / GCNModel build it for "
                "edge_gate='proj' / 'free')")
        if edge_gate == 'proj':
            self.edge_gate = EdgeGateProj(out_channels, in_edgedim=in_edgedim, bias=True)
        elif edge_gate == 'free':
            assert 'num_edges' in kwargs  # a fixed number of edges (gcn_base_models.py:60)
            self.edge_gate = EdgeGateFree(kwargs['num_edges'])
        else:
            self.register_parameter('edge_gate', None)

    _gated = False  # NodeModelGatedAdditive: True

    @staticmethod
    def degnorm_const(edge_index=None, num_nodes=None, deg=None, edge_weight=None, method='sm',
                      device=None):
        """Normalisation constants exactly as gcn_base_models.py:65-146 returns
        them (size (E,), or (N,) for 'rw' without edge weights), computed by
        libmgcn (mgcn_degree_norm / mgcn_edge_norm) and returned in COO order;
        differentiable in edge_weight / deg when they require grad."""
        assert method in ['sm', 'rw']
        if edge_weight is None and deg is None:
            assert edge_index is not None and num_nodes is not None
        plan = plan_for(edge_index, int(num_nodes if num_nodes is not None else deg.numel()))
        norm = plan.norm(method, deg=deg, edge_weight=edge_weight)
        if method == 'rw' and edge_weight is None:
            return norm.dinv  # (with its autograd history when deg requires grad)
        eid = plan.fwd.eid.long()
        if norm.grad:
            return torch.zeros_like(norm.w_fwd).index_put((eid,), norm.w_fwd)
        out = torch.empty_like(norm.w_fwd)
        out[eid] = norm.w_fwd
        return out

    def forward(self, x, edge_index, edge_attr=None, deg=None, *args, **kwargs):
        return x

    def num_parameters(self):
        if not hasattr(self, 'num_para'):
            self.num_para = sum([p.nelement() for p in self.parameters()])
        return self.num_para

    def __repr__(self):
        return '{} (in_channels: {}, out_channels: {}, in_edgedim: {}, deg_norm: {}, edge_gate: {},' \
               'aggr: {} | number of parameters: {})'.format(
                   self.__class__.__name__, self.in_channels, self.out_channels, self.in_edgedim,
                   self.deg_norm, self.edge_gate.__class__.__name__, self.aggr,
                   self.num_parameters())


class NodeModelAdditive(NodeModelBase):
    """gcn_base_models.py:163-243: x @ W, normalised gather, reduce, + bias."""

    def __init__(self, in_channels, out_channels, in_edgedim=None, deg_norm='sm', edge_gate=None,
                 aggr='add', bias=True, **kwargs):
        super().__init__(in_channels, out_channels, in_edgedim, deg_norm, edge_gate, aggr,
                         **kwargs)
        self.weight_node = Parameter(torch.Tensor(in_channels, out_channels))
        if in_edgedim is not None:
            self.weight_edge = Parameter(torch.Tensor(in_edgedim, out_channels))
        if bias:
            self.bias = Parameter(torch.Tensor(out_channels))
        else:
            self.register_parameter('bias', None)
        self.reset_parameters()

    def reset_parameters(self):
        glorot(self.weight_node)
        if self.in_edgedim is not None:
            glorot(self.weight_edge)
        if self.bias is not None:
            zeros(self.bias)

    def forward(self, x, edge_index, edge_attr=None, deg=None, edge_weight=None, **kwargs):
        return self.forward_fused(x, edge_index, edge_attr, deg, edge_weight, relu=False)

    def forward_fused(self, x, edge_index, edge_attr=None, deg=None, edge_weight=None,
                      relu=False):
        """forward() with the caller's ReLU folded into the aggregation epilogue."""
        if edge_attr is not None:
            self._check_edge_attr(edge_attr, edge_index.size(1))
        plan = plan_for(edge_index, x.size(0))
        # deg_norm None ignores edge_weight entirely (gcn_base_models.py:209-211)
        norm = plan.norm(self.deg_norm, deg=deg,
                         edge_weight=edge_weight if self.deg_norm is not None else None)
        if edge_attr is not None:
            y = aggregate_plan(linear(x, self.weight_node), plan, norm, self.aggr)
            return self._add_edge_messages(y, None, edge_attr, edge_index, relu)
        if self.aggr != 'max':
            # torch.matmul(x, W) (gcn_base_models.py:201) fused behind the
            # aggregation where the kernels apply
            return gcn_layer(x, self.weight_node, plan, norm, self.aggr, self.bias, relu)
        x = linear(x, self.weight_node)  # torch.matmul(x, W), gcn_base_models.py:201
        return aggregate_plan(x, plan, norm, self.aggr, self.bias, relu)

    def _check_edge_attr(self, edge_attr, num_edges):
        assert self.in_edgedim is not None  # gcn_base_models.py:205
        if self.aggr == 'max':
            raise NotImplementedError(
                "aggr='max' with an edge_attr message term (gcn_base_models.py:204-227) is not "
                "supported by the mgcn engine: max is not linear in the message, so the term "
                "cannot be aggregated apart from the node rows")
        if edge_attr.dim() != 2 or edge_attr.size(0) != num_edges:
            raise ValueError(f"edge_attr must be [{num_edges}, {self.in_edgedim}], got "
                             f"{tuple(edge_attr.shape)}")

    def _add_edge_messages(self, y, g_coo, edge_attr, edge_index, relu):
        """The edge-feature term of the messages (gcn_base_models.py:204-227)
        by linearity of add / mean:  reduce_k g_k (edge_attr_k @ weight_edge) =
        (reduce_k g_k edge_attr_k) @ weight_edge  (``g_coo`` None: ones), then
        the bias, once, and the caller's ReLU."""
        ea = edge_attr.to(torch.float32)
        if g_coo is not None:
            ea = g_coo.unsqueeze(1) * ea
        ye = linear(scatter_(self.aggr, ea, edge_index[1], y.size(0)),
                    self.weight_edge.to(torch.float32))  # (a bf16 module: cast through autograd)
        y = y + ye.to(y.dtype)
        if self.bias is not None:
            y = y + self.bias.to(y.dtype)
        return torch.relu(y) if relu else y


# ------------------------------------------------ gcn_base_models.py:322-396
class EdgeGateProj(nn.Module):
    """gcn_base_models.py:322-369: a sigmoid gate per edge from the projected
    source row, target row and (optionally) edge features, plus a scalar bias.
    Inside :class:`NodeModelGatedAdditive` the gate is formed in the gather
    kernel; the standalone ``forward`` returns it as [E, 1] in COO order."""

    def __init__(self, in_channels, in_edgedim=None, bias=False):
        super().__init__()
        self.in_channels = in_channels
        self.in_edgedim = in_edgedim
        self.linsrc = nn.Linear(in_channels, 1, bias=False)
        self.lintgt = nn.Linear(in_channels, 1, bias=False)
        if in_edgedim is not None:
            self.linedge = nn.Linear(in_edgedim, 1, bias=False)
        if bias:
            self.bias = Parameter(torch.Tensor(1))  # a scalar bias applied to all edges
        else:
            self.register_parameter('bias', None)
        self.reset_parameters()

    def reset_parameters(self, initrange=0.1):
        nn.init.uniform_(self.linsrc.weight, -initrange, initrange)
        nn.init.uniform_(self.lintgt.weight, -initrange, initrange)
        if self.in_edgedim is not None:
            nn.init.uniform_(self.linedge.weight, -initrange, initrange)
        if self.bias is not None:
            nn.init.constant_(self.bias, 0)

    def gate_terms(self, edge_attr, num_edges):
        """(w_src, w_dst, t) of :func:`mgcn.ops.gate_aggregate`: t holds the
        edge-feature projection and the bias (one element without edge
        features, so the kernel reads it from the device).  The parameters
        go as they are, fp32 or -- a module after ``.to(torch.bfloat16)`` --
        bf16: gate_aggregate casts them to fp32 through autograd."""
        t = self.bias
        if edge_attr is not None:
            assert self.in_edgedim is not None  # gcn_base_models.py:364
            t = linear_bias(edge_attr.to(torch.float32), self.linedge.weight.to(torch.float32),
                            None).view(-1)
            if self.bias is not None:
                t = t + self.bias
        return self.linsrc.weight, self.lintgt.weight, t

    def forward(self, x, edge_index, edge_attr=None, edge_weight=None):
        # A rarely used path (the node model forms its gates in the gather
        # kernel): it runs the whole gated aggregation, the Y gather over all
        # C included, only to return g, and so inherits its C <= 1024 limit.
        plan = plan_for(edge_index, x.size(0))
        w_src, w_dst, t = self.gate_terms(edge_attr, plan.nnz)
        g = gate_aggregate(x, plan, plan.norm(None), 'add', w_src, w_dst, t)[1]
        return g.view(-1, 1)


class EdgeGateFree(nn.Module):
    """gcn_base_models.py:372-396: one free gate parameter per edge (a fixed
    number of edges, in COO order)."""

    def __init__(self, num_edges):
        super().__init__()
        self.num_edges = num_edges
        self.edge_gates = Parameter(torch.Tensor(num_edges, 1))
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.constant_(self.edge_gates, 1)

    def check_edges(self, num_edges):
        if num_edges != self.num_edges:
            raise ValueError(f"EdgeGateFree holds {self.num_edges} gates, the graph has "
                             f"{num_edges} edges")

    def gate_terms(self, edge_attr, num_edges):
        self.check_edges(num_edges)
        return None, None, self.edge_gates.view(-1)

    def forward(self, *args, **kwargs):
        # standalone: no graph is given, so this is the parameter's own sigmoid
        # (inside NodeModelGatedAdditive the gate kernel forms it per slot)
        return torch.sigmoid(self.edge_gates)  # size (E, 1)


class NodeModelGatedAdditive(NodeModelAdditive):
    """gcn_base_models.py:163-243 with ``edge_gate`` 'proj' / 'free': every
    message is multiplied by a learnt sigmoid gate of its edge.  Same
    constructor, parameter names and forward signature as the reference's
    NodeModelAdditive (``num_edges`` in ``**kwargs`` for 'free').  ``x @ W``
    runs on :func:`mgcn.ops.linear`, the gate, the gather, the reduce, bias
    and ReLU on :func:`mgcn.ops.gate_aggregate`; the gate needs the projected
    rows themselves, so the layer is never reassociated to ``(A x) W``.  A
    bfloat16 ``x`` keeps bf16 rows through the gate kernels (fp32 master
    parameters, or the module after ``.to(torch.bfloat16)``) and gives a
    bfloat16 output; the gates stay fp32."""

    _gated = True

    def forward(self, x, edge_index, edge_attr=None, deg=None, edge_weight=None, gate_store=None,
                **kwargs):
        """``gate_store`` (a list) receives this call's gates, [E] in COO edge
        order, detached."""
        return self.forward_fused(x, edge_index, edge_attr, deg, edge_weight, relu=False,
                                  gate_store=gate_store)

    def forward_fused(self, x, edge_index, edge_attr=None, deg=None, edge_weight=None,
                      relu=False, gate_store=None):
        if self.edge_gate is None:
            return super().forward_fused(x, edge_index, edge_attr, deg, edge_weight, relu)
        if edge_attr is not None:
            self._check_edge_attr(edge_attr, edge_index.size(1))
        if isinstance(self.edge_gate, EdgeGateFree):
            self.edge_gate.check_edges(edge_index.size(1))
        plan = plan_for(edge_index, x.size(0))
        norm = plan.norm(self.deg_norm, deg=deg,
                         edge_weight=edge_weight if self.deg_norm is not None else None)
        w_src, w_dst, t = self.edge_gate.gate_terms(edge_attr, plan.nnz)
        hx = linear(x, self.weight_node)  # torch.matmul(x, W), gcn_base_models.py:201
        if edge_attr is None:
            y, g = gate_aggregate(hx, plan, norm, self.aggr, w_src, w_dst, t, self.bias, relu)
        else:
            y, g = gate_aggregate(hx, plan, norm, self.aggr, w_src, w_dst, t)
            y = self._add_edge_messages(y, g, edge_attr, edge_index, relu)
        if gate_store is not None:
            gate_store.append(g.detach())
        return y


# ------------------------------------------------------ graph_attention.py
def _edge_rng(edge_rng):
    """The ``edge_rng`` keyword of the attention modules: 'torch' (the
    reference's draws: ``gumbel_samples`` on the CPU and ``F.dropout``, carried
    to slot order by the op) or 'device' (seeded descriptors the op generates
    on the device in slot order: :class:`mgcn.ops.DeviceGumbel` /
    :class:`mgcn.ops.DeviceDropout` under :func:`mgcn.ops.draw_edge_seed`)."""
    if edge_rng not in ('torch', 'device'):
        raise ValueError(f"edge_rng must be 'torch' or 'device', got {edge_rng!r}")
    return edge_rng


def _combine_heads(y, nheads, channels_1head, combine, bias):
    """The head combine ('cat': none) and the bias after an attention op
    (graph_attention.py:102-117).  bf16 rows (a bf16 ``x``): both are
    accumulated in fp32 from the op's bf16 ``y`` and the result is rounded
    once, so the output keeps the dtype of ``x`` whatever the bias's."""
    rows = y.dtype
    if rows != torch.float32 and (combine != 'cat' or bias is not None):
        y = y.float()
    if combine == 'add':
        y = y.view(-1, nheads, channels_1head).sum(dim=1)
    elif combine == 'mean':
        y = y.view(-1, nheads, channels_1head).mean(dim=1)
    if bias is not None:
        y = y + bias
    return y if y.dtype == rows else y.to(rows)


class NodeModelAttention(NodeModelBase):
    """graph_attention.py:11-123: multi-head soft attention over a node's
    neighbourhood.  ``x @ W`` runs on :func:`mgcn.ops.linear`; scores, the
    per-neighbourhood softmax, the dropout mask and the per-head weighted
    gather are :func:`mgcn.ops.attention_aggregate`.  As in the reference,
    deg_norm / edge_gate / aggr keep NodeModelBase's defaults and are unused,
    and with ``att_combine='cat'`` one head has out_channels / nheads channels
    (else out_channels each).  A bf16 ``x`` keeps bf16 rows through the op
    (fp32 master parameters or a module after ``.to(torch.bfloat16)``) and
    gives a bf16 output; fp32 is the reference's arithmetic.
    ``edge_rng='device'`` (:func:`_edge_rng`; default 'torch') has the
    training dropout mask generated on the device, seeded from torch's CPU
    generator."""

    def __init__(self, in_channels, out_channels, in_edgedim=None, nheads=1, att_act='none',
                 att_dropout=0, att_combine='cat', att_dir='in', bias=False, edge_rng='torch',
                 **kwargs):
        assert att_act in ['none', 'lrelu', 'relu']
        assert att_combine in ['cat', 'add', 'mean']
        assert att_dir in ['in', 'out']
        super().__init__(in_channels, out_channels, in_edgedim)
        self.edge_rng = _edge_rng(edge_rng)
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

    def forward(self, x, edge_index, edge_attr=None, deg=None, edge_weight=None, attn_store=None,
                **kwargs):
        """'deg' and 'edge_weight' are not used (as in the reference).
        ``attn_store`` (a list) receives this call's attention coefficients
        after dropout, [E, nheads] in COO edge order, detached."""
        plan = plan_for(edge_index, x.size(0))
        hp = linear(x, self.weight)
        mask = None
        if self.training and self.att_dropout.p > 0 and self.edge_rng == 'device':
            mask = DeviceDropout(self.att_dropout.p, *draw_edge_seed())
        elif self.training and self.att_dropout.p > 0:
            # the reference's Dropout on alpha: alpha * mask with mask = dropout(ones)
            mask = nn.functional.dropout(
                torch.ones(plan.nnz, self.nheads, dtype=torch.float32, device=hp.device),
                p=self.att_dropout.p, training=True)
        y, alpha = attention_aggregate(hp, self.att_weight, plan, self.nheads,
                                       self.att_act_name, self.att_dir, edge_mask=mask)
        y = _combine_heads(y, self.nheads, self.out_channels_1head, self.att_combine, self.bias)
        if attn_store is not None:
            attn_store.append(alpha)
        return y

    def __repr__(self):
        return ('{} (in_channels: {}, out_channels: {}, in_edgedim: {}, nheads: {}, '
                'att_activation: {},att_dropout: {}, att_combine: {}, att_dir: {} | '
                'number of parameters: {}').format(
                    self.__class__.__name__, self.in_channels, self.out_channels,
                    self.in_edgedim, self.nheads, self.att_act, self.att_dropout.p,
                    self.att_combine, self.att_dir, self.num_parameters())


# ------------------------------------------------- graph_hard_attention.py
def gumbel_samples(base):
    """graph_hard_attention.py:12-20: iid Gumbel(0, 1) samples with the size,
    dtype and device of ``base``.  NodeModelHardAttention.forward calls it
    through this module global, once, with a float32 [E, nheads] tensor, and
    reads the result in COO edge order (tests replace the global to replay
    recorded noise)."""
    noise = torch.rand(base.size()).to(base)
    eps = 1e-20
    noise.add_(eps).log_().neg_()
    noise.add_(eps).log_().neg_()
    return noise


class NodeModelHardAttention(NodeModelBase):
    """graph_hard_attention.py:23-163: multi-head hard attention over a
    node's neighbourhood.  Training is the Gumbel-softmax relaxation (noise
    and a temperature inside the softmax logits, dropout on the coefficients);
    eval keeps, per node and head, the single neighbour with the largest score
    (plus Gumbel noise when ``sample``).  ``x @ W`` runs on
    :func:`mgcn.ops.linear`, everything after it on
    :func:`mgcn.ops.hard_attention_aggregate`, which also mirrors the
    reference's last-edge quirk for nodes without a neighbour.  Head widths
    follow ``att_combine`` as in :class:`NodeModelAttention`.
    ``edge_rng='device'`` (:func:`_edge_rng`; default 'torch') has the Gumbel
    noise (training, and eval with ``sample``) and the training dropout mask
    generated on the device, seeded from torch's CPU generator: no CPU draw,
    no host-to-device copy, and ``gumbel_samples`` is not called."""

    def __init__(self, in_channels, out_channels, in_edgedim=None, nheads=1, att_act='none',
                 att_dropout=0, att_combine='cat', att_dir='in', bias=False, temperature=0.1,
                 sample=False, edge_rng='torch', **kwargs):
        assert att_act in ['none', 'lrelu', 'relu']
        assert att_combine in ['cat', 'add', 'mean']
        assert att_dir in ['in', 'out']
        super().__init__(in_channels, out_channels, in_edgedim)
        self.edge_rng = _edge_rng(edge_rng)
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

    def forward(self, x, edge_index, edge_attr=None, deg=None, edge_weight=None, attn_store=None,
                **kwargs):
        """'deg' and 'edge_weight' are not used (as in the reference).
        ``attn_store`` (a list) receives the coefficients that weighted the
        messages, [E, nheads] in COO edge order, detached: in training the
        Gumbel-softmax after dropout, in eval the one-hot (with the quirk
        edge)."""
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
        y = _combine_heads(y, self.nheads, self.out_channels_1head, self.att_combine, self.bias)
        if attn_store is not None:
            attn_store.append(alpha)
        return y

    def __repr__(self):
        return ('{} (in_channels: {}, out_channels: {}, in_edgedim: {}, nheads: {}, '
                'att_activation: {},att_dropout: {}, att_combine: {}, att_dir: {}, '
                'temperature: {} | number of parameters: {})').format(
                    self.__class__.__name__, self.in_channels, self.out_channels,
                    self.in_edgedim, self.nheads, self.att_act, self.att_dropout.p,
                    self.att_combine, self.att_dir, self.temperature, self.num_parameters())


# ------------------------------------------------------ gcn_multi_kernel.py
class GCNMultiKernel(nn.Module):
    """gcn_multi_kernel.py:9-114.  The 'additive' and 'attention' node models
    run on this engine; 'hardattention' is not registered here yet
    (:class:`NodeModelHardAttention` exists and is used directly).

    Two to eight plain additive kernels (add / mean, no gate, no edge_attr,
    fp32 rows, no heavy rows, no gradient asked of deg / edge_weight) run as
    one GEMM and one launch per direction (:meth:`_forward_multi`,
    :func:`mgcn.ops.multi_kernel_fusable`); everything else is the loop over
    the node models.  'mean' divides by the number of kernels with edges and
    'cat' concatenates (the reference raises for both when K > 1)."""

    nodemodel_dict = {'additive': NodeModelAdditive, 'attention': NodeModelAttention}

    def __init__(self, *args, num_kernel=1, nodemodel='additive', kernel_combine='add',
                 **kwargs):
        assert nodemodel in ['additive', 'attention', 'hardattention']
        assert kernel_combine in ['add', 'cat', 'mean']
        super().__init__()
        if nodemodel not in self.nodemodel_dict:
            raise NotImplementedError(f"nodemodel={nodemodel!r} is not supported by mgcn")
        self.kernel_combine = kernel_combine
        cls = self.nodemodel_dict[nodemodel]
        edge_gate = kwargs.get('edge_gate', args[4] if len(args) > 4 else None)
        if nodemodel == 'additive' and edge_gate is not None:
            cls = NodeModelGatedAdditive
        self.node_models = nn.ModuleList([cls(*args, **kwargs) for k in range(num_kernel)])

    def reset_parameters(self):
        for net in self.node_models:
            net.reset_parameters()

    @staticmethod
    def _listify(edge_index_K, edge_attr_K, deg_K, edge_weight_K):
        # gcn_multi_kernel.py:77-91
        if isinstance(edge_index_K, torch.Tensor):
            edge_index_K = [edge_index_K]
        if isinstance(edge_attr_K, torch.Tensor):
            edge_attr_K = [edge_attr_K]
        if isinstance(deg_K, torch.Tensor):
            deg_K = [deg_K]
        if isinstance(edge_weight_K, torch.Tensor):
            edge_weight_K = [edge_weight_K]
        n = len(edge_index_K)
        return (edge_index_K, edge_attr_K or [None] * n, deg_K or [None] * n,
                edge_weight_K or [None] * n)

    def forward(self, x, edge_index_K, edge_attr_K=None, deg_K=None, edge_weight_K=None,
                **kwargs):
        return self.forward_fused(x, edge_index_K, edge_attr_K, deg_K, edge_weight_K, relu=False,
                                  **kwargs)

    def can_fuse_relu(self, edge_index_K) -> bool:
        """The layer's ReLU can ride in forward_fused: a single additive kernel
        (its aggregation's epilogue), or a module the fused multi-kernel route
        may take (there the ReLU follows the combine in the launch; a call the
        route declines applies it after the loop)."""
        if isinstance(edge_index_K, torch.Tensor):
            edge_index_K = [edge_index_K]
        if len(self.node_models) == 1 and len(edge_index_K) == 1:
            return edge_index_K[0] is not None \
                and all(isinstance(nm, NodeModelAdditive) for nm in self.node_models)
        nms = [nm for nm, ei in zip(self.node_models, edge_index_K) if ei is not None]
        return _ops._FUSE_MULTI and 2 <= len(nms) <= L.MULTI_MAX_K \
            and all(type(nm) is NodeModelAdditive and nm.aggr in ('add', 'mean') for nm in nms)

    def _multi_reason(self, x, eis, eas):
        """:func:`mgcn.ops.multi_kernel_reason` of this module on this call
        (what is known before a plan is built)."""
        nms = [nm for nm, ei in zip(self.node_models, eis) if ei is not None]
        return multi_kernel_reason(
            x, len(nms), nms[0].aggr if nms else 'add',
            plain=all(type(nm) is NodeModelAdditive for nm in nms),
            edge_attr=any(ea is not None for ei, ea in zip(eis, eas) if ei is not None))

    def _forward_multi(self, x, eis, eas, degs, ews, relu):
        """The K kernels in one launch per direction (gcn_multi_kernel.py:93-112
        on :func:`mgcn.ops.multi_aggregate`): one GEMM x @ [W_0 | .. | W_{K-1}]
        reads x once, the kernels' results are combined (and the ReLU applied)
        in registers, and the backward is one adjoint launch and one dense
        backward.  None when the route does not apply
        (:func:`mgcn.ops.multi_kernel_fusable`): the caller runs the loop."""
        if not _ops._FUSE_MULTI or self._multi_reason(x, eis, eas) is not None \
                or _wants_norm_grad(degs, ews):
            return None
        present = [t for t in zip(self.node_models, eis, degs, ews) if t[1] is not None]
        nms = [t[0] for t in present]
        plans = [plan_for(ei, x.size(0)) for _, ei, _, _ in present]
        # deg_norm None ignores edge_weight entirely (gcn_base_models.py:209-211)
        norms = [plan.norm(nm.deg_norm, deg=deg, edge_weight=ew if nm.deg_norm is not None else None)
                 for plan, (nm, _, deg, ew) in zip(plans, present)]
        if not multi_kernel_fusable(x, plans, norms, nms[0].aggr,
                                    out_channels=nms[0].out_channels):
            return None
        h_all = linear(x, torch.cat([nm.weight_node for nm in nms], dim=1))
        return multi_aggregate(h_all, plans, norms, [nm.bias for nm in nms], nms[0].aggr,
                               self.kernel_combine, relu)

    def forward_fused(self, x, edge_index_K, edge_attr_K=None, deg_K=None, edge_weight_K=None,
                      relu=False, **kwargs):
        eis, eas, degs, ews = self._listify(edge_index_K, edge_attr_K, deg_K, edge_weight_K)
        if relu:
            assert self.can_fuse_relu(edge_index_K)
        if relu and len(self.node_models) == 1:
            nm = self.node_models[0]
            if isinstance(nm, NodeModelGatedAdditive):
                return nm.forward_fused(x, eis[0], eas[0], degs[0], ews[0], relu=True,
                                        gate_store=kwargs.get('gate_store'))
            return nm.forward_fused(x, eis[0], eas[0], degs[0], ews[0], relu=True)
        if len(self.node_models) > 1:
            y = self._forward_multi(x, eis, eas, degs, ews, relu)
            if y is not None:
                return y
        xo = self._forward_loop(x, eis, eas, degs, ews, **kwargs)
        return torch.relu(xo) if relu else xo

    def _forward_loop(self, x, eis, eas, degs, ews, **kwargs):
        """One node model call per kernel, combined as gcn_multi_kernel.py:93-112."""
        xo = None
        outs = []
        for nm, edge_index, edge_attr, deg, edge_weight in zip(self.node_models, eis, eas, degs,
                                                               ews):
            if edge_index is None:
                continue
            if isinstance(nm, NodeModelAttention):
                y = nm(x, edge_index, edge_attr, deg, edge_weight, **kwargs)  # attn_store
            elif isinstance(nm, NodeModelGatedAdditive):
                y = nm(x, edge_index, edge_attr, deg, edge_weight,
                       gate_store=kwargs.get('gate_store'))
            else:
                y = nm(x, edge_index, edge_attr, deg, edge_weight)
            outs.append(y)
        if not outs:
            return 0
        if self.kernel_combine == 'cat':
            # the reference's `xo != 0` test breaks for K > 1 (gcn_multi_kernel.py:100);
            # the intended concatenation is done here
            return torch.cat(outs, dim=1)
        xo = outs[0]
        for y in outs[1:]:
            xo = xo + y
        if self.kernel_combine == 'mean':
            xo = xo / len(outs)
        return xo


# -------------------------------------------------------------- gcn_model.py
class GCNLayer(nn.Module):
    """gcn_model.py:128-197; a ReLU layer activation is fused into the
    aggregation epilogue when there is a single kernel, and into the fused
    multi-kernel launch (after the combine) when there are several plain
    additive ones (:meth:`GCNMultiKernel.can_fuse_relu`)."""

    def __init__(self, in_channels, out_channels, in_edgedim=None, deg_norm='sm', edge_gate=None,
                 aggr='add', bias=True, num_kernel=1, nodemodel='additive', non_linear='relu',
                 **kwargs):
        super().__init__()
        if nodemodel != 'attention':
            kwargs.pop('nheads', None)  # attention-only argument (gcn_model.py:49)
        self.gcn = GCNMultiKernel(in_channels, out_channels, in_edgedim, deg_norm=deg_norm,
                                  edge_gate=edge_gate, aggr=aggr, bias=bias,
                                  num_kernel=num_kernel, nodemodel=nodemodel, **kwargs)
        self.non_linear = activation(non_linear)
        self.non_linear_name = non_linear
        self._relu = non_linear == 'relu'

    def reset_parameters(self):
        self.gcn.reset_parameters()

    def forward(self, x, edge_index_K, edge_attr_K=None, deg_K=None, edge_weight_K=None,
                **kwargs):
        if self._relu and self.gcn.can_fuse_relu(edge_index_K):
            return self.gcn.forward_fused(x, edge_index_K, edge_attr_K, deg_K, edge_weight_K,
                                          relu=True, **kwargs)  # gate_store
        xo = self.gcn(x, edge_index_K, edge_attr_K, deg_K, edge_weight_K, **kwargs)
        return self.non_linear(xo)


class GCNStack(nn.Module):
    """A plain chain of GCNLayers (the config-2 model: 3 layers, ReLU between)
    executed as ONE fused autograd node (:func:`mgcn.ops.gcn_stack`) whenever
    every layer is a single additive kernel with the same deg_norm/aggr and a
    'relu'/'none' activation; otherwise layer by layer.  Parameters live in
    the GCNLayer modules (reference-compatible state_dict keys)."""

    def __init__(self, layers):
        super().__init__()
        self.layers = nn.ModuleList(layers)

    def _fusable(self, x=None):
        if x is not None and x.dtype != torch.float32:
            return None  # bf16 activations: layer by layer through gcn_layer
        nms = []
        for layer in self.layers:
            g = layer.gcn
            if len(g.node_models) != 1 or layer.non_linear_name not in ('relu', 'none'):
                return None
            if not isinstance(g.node_models[0], NodeModelAdditive):
                return None  # attention layers: layer by layer
            if g.node_models[0].edge_gate is not None:
                return None  # gated layers: layer by layer (the gate reads x W itself)
            nms.append(g.node_models[0])
        if len({(nm.deg_norm, nm.aggr) for nm in nms}) != 1:
            return None
        return nms

    def forward(self, x, edge_index, deg=None, edge_weight=None):
        nms = self._fusable(x)
        if nms is None or x.device.type != "cuda":
            for layer in self.layers:
                x = layer(x, edge_index, None, deg, edge_weight)
            return x
        plan = plan_for(edge_index, x.size(0))
        norm = plan.norm(nms[0].deg_norm, deg=deg,
                         edge_weight=edge_weight if nms[0].deg_norm is not None else None)
        relus = [layer.non_linear_name == 'relu' for layer in self.layers]
        return gcn_stack(x, plan, norm, [nm.weight_node for nm in nms], [nm.bias for nm in nms],
                         relus, nms[0].aggr)


class GCNModel(nn.Module):
    """gcn_model.py:8-125: GCN layers, residual Linear every `residual_hop`
    layers, dropout, optional final projection, optional graph mean-pool."""

    def __init__(self, in_channels, enc_sizes, num_classes, non_linear='relu',
                 non_linear_layer_wise='relu', residual_hop=None, dropout=0.5,
                 final_layer_config=None, final_type='none', pred_on='node', **kwargs):
        assert final_type in ['none', 'proj']
        assert pred_on in ['node', 'graph']
        super().__init__()
        self.in_channels = in_channels
        self.enc_sizes = [in_channels, *enc_sizes]
        self.num_layers = len(self.enc_sizes) - 1
        self.num_classes = num_classes
        self.residual_hop = residual_hop
        self.non_linear_layer_wise = non_linear_layer_wise
        self.final_type = final_type
        self.pred_on = pred_on
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
        if final_layer_config is None:
            self.gcn_net = nn.ModuleList([
                GCNLayer(in_c, out_c, nheads=nh, non_linear=non_linear_layer_wise, **kwargs)
                for in_c, out_c, nh in zip(self.enc_sizes, self.enc_sizes[1:], self.nheads)])
        else:
            assert isinstance(final_layer_config, dict)
            self.gcn_net = nn.ModuleList([
                GCNLayer(in_c, out_c, nheads=nh, non_linear=non_linear_layer_wise, **kwargs)
                for in_c, out_c, nh in zip(self.enc_sizes[:-2], self.enc_sizes[1:-1],
                                           self.nheads[:-1])])
            kwargs.update(final_layer_config)
            self.gcn_net.append(GCNLayer(self.enc_sizes[-2], self.enc_sizes[-1],
                                         nheads=self.nheads[-1],
                                         non_linear=non_linear_layer_wise, **kwargs))
        self.dropout = nn.Dropout(dropout)
        if residual_hop is not None and residual_hop > 0:
            self.residuals = nn.ModuleList([
                Linear(self.enc_sizes[i], self.enc_sizes[j])
                for i, j in zip(range(0, len(self.enc_sizes), residual_hop),
                                range(residual_hop, len(self.enc_sizes), residual_hop))])
            self.non_linear = activation(non_linear)
            self.num_residuals = len(self.residuals)
        if self.final_type == 'none':
            self.final = nn.Identity()
        elif self.final_type == 'proj':
            self.final = Linear(self.enc_sizes[-1], num_classes)
        else:
            raise ValueError

    def reset_parameters(self):
        for net in self.gcn_net:
            net.reset_parameters()
        if self.residual_hop is not None:
            for net in self.residuals:
                net.reset_parameters()
        if self.final_type != 'none':
            self.final.reset_parameters()

    fuse_residual = True  # class switch (tests compare against the step-for-step path)

    def _residual_fusable(self, x, edge_index_K, edge_attr_K):
        """residual_hop = 1 with single additive kernels, ReLU joins and no
        active dropout: each layer + its residual runs as one fused node."""
        if not self.fuse_residual or self.residual_hop != 1 or \
                getattr(self, 'num_residuals', 0) != self.num_layers:
            return False
        if not isinstance(edge_index_K, torch.Tensor) or edge_attr_K is not None:
            return False
        if x.device.type != "cuda" or not isinstance(self.non_linear, nn.ReLU):
            return False
        if x.dtype != torch.float32:
            return False  # bf16 activations: step for step
        if self.training and self.dropout.p > 0:
            return False
        for layer in self.gcn_net:
            if len(layer.gcn.node_models) != 1 or layer.non_linear_name not in ('relu', 'none'):
                return False
            if not isinstance(layer.gcn.node_models[0], NodeModelAdditive):
                return False  # attention layers: step for step
            if layer.gcn.node_models[0].edge_gate is not None:
                return False  # gated layers: step for step
        return True

    def forward(self, x, edge_index_K, edge_attr_K=None, deg_K=None, edge_weight_K=None,
                **kwargs):
        if (self._residual_fusable(x, edge_index_K, edge_attr_K) and
                not _wants_norm_grad(deg_K, edge_weight_K)):
            x = self._forward_residual_fused(x, edge_index_K, deg_K, edge_weight_K)
            return self._readout(x, **kwargs)
        # gcn_model.py:86-125, step for step
        xr = None
        add_xr_at = -1
        for n, net in enumerate(self.gcn_net):
            xo = net(x, edge_index_K, edge_attr_K, deg_K, edge_weight_K, **kwargs)
            xo = self.dropout(xo)
            if self.residual_hop is not None and self.residual_hop > 0:
                if n % self.residual_hop == 0 and (n // self.residual_hop) < self.num_residuals:
                    xr = self.residuals[n // self.residual_hop](x)
                    add_xr_at = n + self.residual_hop - 1
                if n == add_xr_at:
                    if n < self.num_layers - 1:
                        xo = self.non_linear(xo + xr)
                    else:
                        xo = xo + xr
            x = xo
        return self._readout(x, **kwargs)

    def _forward_residual_fused(self, x, edge_index, deg, edge_weight):
        if isinstance(deg, (list, tuple)):
            deg = deg[0]
        if isinstance(edge_weight, (list, tuple)):
            edge_weight = edge_weight[0]
        plan = plan_for(edge_index, x.size(0))
        last = self.num_layers - 1
        items = []
        for n, (layer, res) in enumerate(zip(self.gcn_net, self.residuals)):
            nm = layer.gcn.node_models[0]
            norm = plan.norm(nm.deg_norm, deg=deg,
                             edge_weight=edge_weight if nm.deg_norm is not None else None)
            items.append((nm, norm, layer.non_linear_name == 'relu', n < last, res))
        n = 0
        while n < len(items):
            nm, norm, relu1, relu2, res = items[n]
            # a run of 32 -> 32 layers on the same normalisation and aggregator:
            # one fused stack node (one host call per direction)
            m = n
            while (m < len(items) and items[m][1] is norm and items[m][0].aggr == nm.aggr and
                   residual_layer_supported(plan, x, items[m][0].weight_node,
                                            items[m][4].weight, L.REDUCE_CODES[nm.aggr])):
                m += 1
            if m - n >= 2:
                x = residual_stack(x, plan, norm, nm.aggr, [it[2] for it in items[n:m]],
                                   [it[3] for it in items[n:m]],
                                   [(it[0].weight_node, it[0].bias, it[4].weight, it[4].bias)
                                    for it in items[n:m]])
                n = m
                continue
            x = residual_gcn_layer(x, plan, norm, nm.aggr, relu1, relu2, nm.weight_node, nm.bias,
                                   res.weight, res.bias)
            n += 1
        return x

    def _readout(self, x, **kwargs):
        x = self.final(x)
        if self.pred_on == 'graph':
            assert 'batch_slices_x' in kwargs
            batch_slices_x = kwargs['batch_slices_x']
            if len(batch_slices_x) == 2:
                x = x.mean(dim=0, keepdim=True)
            else:
                x_batch, lengths = zip(*[(x[i:j], j - i) for (i, j) in
                                         zip(batch_slices_x, batch_slices_x[1:])])
                x_batch = pad_sequence(x_batch, batch_first=True, padding_value=0)
                x = x_batch.sum(dim=1) / x_batch.new_tensor(lengths)
        return x


__all__ = ["glorot", "zeros", "Identity", "activation", "scatter_", "Linear", "NodeModelBase",
           "NodeModelAdditive", "EdgeGateProj", "EdgeGateFree", "NodeModelGatedAdditive",
           "NodeModelAttention", "NodeModelHardAttention",
           "GCNMultiKernel", "GCNLayer", "GCNStack", "GCNModel"]
_ = L  # keep the binding imported so a missing library fails at import of ops
