"""control_gic_amd -- MI355X (gfx950) implementation of Control-GIC's
granularity-adaptive VQ + router + entropy-coder hot path behind the
reference's own module API (see DESIGN.md / INTEGRATION.md).

Import name: `control_gic_amd` (the directory is `control-gic_amd/`; the
root-level control_gic_amd.py maps one to the other).
"""
from . import _lib
from ._lib import CgicError, LIB_PATH
from .quantize import VectorQuantize2, VectorQuantizer
from .router import TripleGrainFixedEntropyRouter
from .entropy import Entropy, entropy_maps, entropy_maps_u8, entropy_maps_tiles
from .indices_coding import HuffmanCoding
from .mask_coding import BinaryCoding
from .codec import GrainCodec, CompressedBatch, mode_streams, STREAM_NAMES, decoder_mode
from . import pipeline, highres, container, draw, ema, adam, model, norm, resblock, ops, experimental
from .pipeline import HotPathPipeline, LaneStream, GraphLanes, capture_graph
from .model import install, compress_batch, grain_merge, avg_pool, decoder_blend_medium, decoder_blend_fine
from . import rate
from .norm import SpatialNorm, spatial_norm, spatial_norm_backward, spatial_norm_train
from .norm import GroupNorm, group_norm, group_norm_backward, group_norm_train
from .resblock import ResnetBlock
from .attention import AttnBlock, attention, attention_backward
from .ema import LitEma, EmaPlan
from .adam import Adam, AdamPlan
from .rate import RateTable, rate_table, grain_indices, gather_grain_indices, choose, default_candidates, compress_to_bpp
from .rate import RateCurve, rate_curve, ratio_for_rank, router_ranks
from .rate import BppRoute, budget_bytes, route_to_bpp
from .highres import to_frames, paste_tiles, partition_tiles
from .draw import partition_map, grain_map, draw_triple_grain_256res
from .rate import TiledRateCurve, rate_curve_tiled, tiled_settings, compress_tiled_to_bpp

__all__ = ["VectorQuantize2", "VectorQuantizer", "TripleGrainFixedEntropyRouter", "Entropy", "entropy_maps", "entropy_maps_u8", "entropy_maps_tiles",
           "HuffmanCoding", "BinaryCoding", "GrainCodec", "CompressedBatch", "mode_streams", "STREAM_NAMES",
           "HotPathPipeline", "LaneStream", "GraphLanes", "capture_graph", "decoder_mode", "install", "compress_batch", "grain_merge", "avg_pool", "decoder_blend_medium", "decoder_blend_fine", "rate", "RateTable", "rate_table", "grain_indices", "gather_grain_indices", "choose",
           "default_candidates", "compress_to_bpp", "RateCurve", "rate_curve", "ratio_for_rank", "router_ranks",
           "BppRoute", "budget_bytes", "route_to_bpp",
           "TiledRateCurve", "rate_curve_tiled", "tiled_settings", "compress_tiled_to_bpp", "to_frames", "paste_tiles", "partition_tiles", "partition_map", "grain_map", "draw_triple_grain_256res", "draw", "highres", "container", "norm", "SpatialNorm", "spatial_norm", "spatial_norm_train", "spatial_norm_backward", "GroupNorm", "group_norm", "group_norm_train", "group_norm_backward", "resblock", "ResnetBlock", "AttnBlock", "attention", "attention_backward", "ema", "LitEma", "EmaPlan", "adam", "Adam", "AdamPlan", "CgicError", "LIB_PATH"]
