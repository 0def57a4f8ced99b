"""pt2q — MI355X-native ternary PTQ calibration engine (PT²-LLM: ATQ + SSR inside a GPTQ loop).

Drop-in for the reference's hot-path surface:
    AsymmetricTernaryQuantizer, compute_quantization_error, compute_output_error  (quantizer.py)
    compute_output_error_from_gram, quadform_rows, layer_report   (the same metrics from the Gram)
    compute_column_similarity_to_mean, select_next_block_ssr,
    compute_cosine_similarity_matrix, get_initial_reorder_indices, SSRReorderer,
    apply_permutation, apply_permutation_to_input, compute_block_variance         (reorder.py)
    GPTQ, GPTQQuantizer                                                            (gptq.py)
    PT2LLMQuantizer.quantize_layer                                                 (main.py)
    pack_ternary, unpack_ternary, save/load_quantized_model,
    compute_bits_per_weight, evaluate_perplexity                                   (utils.py)
    TernaryLinear, replace_linear_with_ternary                                     (model.py)
    ternary_decode, set_decode               (the fused 1-8 token decode kernel of TernaryLinear)
    ternary_decode_group, ternary_decode_swiglu, TernaryGatedMLP, fuse_gated_mlp
                                             (projections sharing x, and gate/up + SwiGLU, in one launch)
    rms_norm, TernaryMLPBlock                (RMSNorm as a kernel and as the decode kernel's prologue,
                                              the residual add as its epilogue: h + mlp(norm(h)) in two launches)
All compute runs in libpt2q.so (HIP, gfx950); importing fails loudly if it is not built.
"""
from . import _lib
from .quantizer import (AsymmetricTernaryQuantizer, compute_output_error, compute_output_error_from_gram,
                        compute_quantization_error, quadform_rows)
from .reorder import (SSRReorderer, apply_permutation, apply_permutation_to_input, compute_block_variance,
                      compute_column_similarity_to_mean, compute_cosine_similarity_matrix,
                      get_initial_reorder_indices, select_next_block_ssr)
from .gptq import GPTQ, GPTQQuantizer
from .pt2llm import PT2LLMQuantizer
from .calibration import (GramAccumulator, GramCapture, find_linear_layers, get_llm_layers,
                          quantize_decoder_layer)
from .ternary import (TernaryGatedMLP, TernaryLinear, TernaryMLPBlock, compute_bits_per_weight, fuse_gated_mlp,
                      load_quantized_model, replace_linear_with_ternary, rms_norm, save_quantized_model, set_decode,
                      ternary_decode, ternary_decode_group, ternary_decode_swiglu)
from .evaluation import evaluate_perplexity
from .engine import (LayerGraph, LayerOutput, LayerWorkspace, UnitRun, UnitWorkspace, cholesky_inverse,
                     dequantize, error_feedback, fill_synthetic, gram, hessian_inverse, pack_ternary, prepare_hessian,
                     quantize_blocks, quantize_layer, quantize_shared, quantize_unit, unpack_ternary,
                     UnitPipeline, sum_partials, LayerReport, layer_report)

__version__ = "0.1.0"
__all__ = [
    "AsymmetricTernaryQuantizer", "compute_quantization_error", "compute_output_error",
    "compute_column_similarity_to_mean", "select_next_block_ssr", "GPTQ", "GPTQQuantizer",
    "PT2LLMQuantizer", "LayerGraph", "LayerOutput", "LayerWorkspace", "gram", "prepare_hessian",
    "cholesky_inverse", "quantize_blocks", "quantize_layer", "dequantize", "pack_ternary",
    "unpack_ternary", "fill_synthetic", "hessian_inverse", "quantize_shared", "GramAccumulator",
    "GramCapture", "find_linear_layers", "get_llm_layers", "quantize_decoder_layer",
    "TernaryLinear", "replace_linear_with_ternary", "save_quantized_model", "load_quantized_model",
    "UnitRun", "UnitWorkspace", "quantize_unit", "compute_bits_per_weight", "error_feedback",
    "UnitPipeline", "sum_partials", "evaluate_perplexity", "compute_cosine_similarity_matrix",
    "get_initial_reorder_indices", "SSRReorderer", "apply_permutation", "apply_permutation_to_input",
    "compute_block_variance", "LayerReport", "layer_report", "quadform_rows", "compute_output_error_from_gram",
    "ternary_decode", "set_decode", "ternary_decode_group", "ternary_decode_swiglu", "TernaryGatedMLP",
    "fuse_gated_mlp", "rms_norm", "TernaryMLPBlock",
]
