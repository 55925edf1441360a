"""mgcn -- MI355X-native GCN message passing (the Â·X aggregation of
jzhou316/meta-gcn) behind the reference's own module surface.

    mgcn.models : gcn_meta surface (NodeModelAdditive, NodeModelAttention,
                  NodeModelHardAttention, NodeModelGatedAdditive, GCNMultiKernel,
                  GCNLayer, GCNModel, scatter_, activation)
    mgcn.pyg    : PyG-1.x surface used by kernel/ (GCNConv, GINConv, SAGEConv,
                  GraphConv, global_mean_pool, JumpingKnowledge)
    mgcn.ops    : fused aggregation autograd ops
    mgcn.graph  : device CSR plans + cache
    mgcn.dist   : destination-range sharding over torch.distributed (RCCL)

All compute goes through libmgcn.so (include/mgcn.h); there is no CPU path.
"""
import torch  # noqa: F401  -- must be imported before libmgcn binds libamdhip64

from . import _lib
from ._lib import MgcnError, check_device, load, set_option
from .graph import (GraphPlan, adopt_plan, build_plan, clear_cache, drop_edges, plan_for,
                    set_derived_plans)
from .ops import (Block, DeviceDropout, DeviceGumbel, aggregate, attention_aggregate,
                  block_aggregate, block_batches, block_convs, draw_edge_seed, edge_noise,
                  gate_aggregate, hard_attention_aggregate, multi_aggregate, sample_blocks, sample_keep,
                  sample_layers, sample_neighbors, scatter_, segment_mean,
                  set_block_convs, set_sample_heavy_rows)

__version__ = "0.1.0"

__all__ = ["MgcnError", "check_device", "load", "set_option", "GraphPlan", "build_plan", "plan_for",
           "clear_cache", "aggregate", "attention_aggregate", "gate_aggregate",
           "multi_aggregate", "hard_attention_aggregate", "scatter_", "segment_mean", "_lib",
           "adopt_plan", "drop_edges", "set_derived_plans", "edge_noise", "DeviceGumbel",
           "DeviceDropout", "draw_edge_seed", "sample_keep", "sample_neighbors", "sample_layers",
           "set_sample_heavy_rows", "Block", "sample_blocks", "block_batches", "block_aggregate",
           "set_block_convs", "block_convs"]
