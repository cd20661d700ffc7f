"""MI355X-native spectral mixing: drop-in for `fft_tensor.spectral_layers.SpectralMixingLayer`
and `fft_tensor.wirtinger_ops` of fricker2025-star/Tensor-Cuda-FFT-.

Import as `tensor_cuda_fft_amd` (the shim at the repo root maps that name onto this directory,
whose on-disk name is not a Python identifier).
"""
from .spectral_layers import HybridSpectralAttention, SpectralMixingLayer, SpectralMLPBlock
from .wirtinger_ops import (ComplexParameter, WirtingerGradient, WirtingerSpectralFilter,
                            spectral_mix_with_filter)
from .functional import (DropoutState, hermitian_scale, irfft, pruned_rfft, rfft, rfft_bins, seq_fft,
                         spectral_block_mix, spectral_filter, spectral_mix, ema_scan, ema_scan_tokens, narrow_head,
                         word_targets, cross_entropy, sample_bytes, byte_features, find_snippets, sparsify_topk,
                         sparse_scatter, fftn, ifftn, frequency_attention, bin_contract, polar_range, polar_quantize,
                         polar_dequantize, log8_encode, log8_decode, log8_encode_complex, log8_decode_complex,
                         rowfft_supported, row_fft_raw, row_fft, row_ifft)
from .spectral_enhancements import (CausalFrequencyMask, EnhancedSpectralBlock, GatedSpectralUnit,
                                    MultiScaleSpectralFeatures, PhaseAwareSpectralMixing, RotaryFrequencyEmbedding)
from .complex_rope import ComplexRoPE, ComplexRoPESpectralLayer, GatedLinearUnit
from .frequency_ops import (ComplexSemanticEmbedding, FrequencyAttention, FrequencyMatMul, FrequencyTransformerLayer,
                            frequency_layernorm, frequency_relu)
from .sparse_tensor import MemoryManager, SparseSpectralTensor, randn_sst, sst, zeros_sst
from .optimized_ops import OptimizedFrequencyOps, ProductionFrequencyLinear
from .production_ready import OptimizedSparseSpectralTensor, ProductionFrequencyOps
from .polar_quantization import PolarQuantizer
from .zero_materialize import (ConvolutionTheoremMatMul, FrequencyLinearLayer, LogarithmicQuantizer, WirtingerAutograd,
                               frequency_conv1d, frequency_linear)
from .llamaizer import FFTConverter
from .ops import spectral_activation, spectral_normalize, spectral_pool
from .fixed_spectral import (FixedSpectralBlock, FixedSpectralLM, FrequencyConvFunc, LMConfig, SampleConfig,
                             causal_spectral_conv, generate)
from .frequency_native import BicameralBlock, FrequencyNativeBlock, PhaseShift, SpectralFFN, SpectralLayerNorm
from .spectral_ssm import EMAConfig, SpectralEMA
from .chunk_head import ChunkLM, vectorized_windows
from .phase_clock import PhaseClockChunkLM, PhaseClockHead, compute_phase_clock_loss, generate_phase_targets
from .segmentation_head import SegmentationHead, SegmentedChunkLM, compute_segmented_loss, get_word_boundaries
from .dual_head import DualHead, TokenAwareChunkLM, compute_dual_loss, get_gpt2_tokenizer, get_token_ids_fast
from .streaming import (LayerStream, StreamStates, generate_chunked, init_layer_states, stream_taps,
                        update_backbone_chunk)
from .byte_spectral import ByteSpectralEmbedding, ByteSpectralEncoder, SpectralLanguageModel
from .distributed import GradSync, attach_grad_sync, all_reduce_grads, shard_batch
from .training import (TrainConfig, adaptive_cutoff, checkpoint_state, config_from_checkpoint, conv_freq_bins,
                       curriculum_cutoff, eval_loss, jpeg_cutoff, load_checkpoint, load_corpus_as_u8, load_state_flexible,
                       lr_stage_params, make_val_starts, parroting_picks, parroting_score, plateau_cutoff, sample_windows,
                       save_checkpoint, sawtooth_lr, verify_checkpoint)

__all__ = [
    "SpectralMixingLayer", "SpectralMLPBlock", "HybridSpectralAttention", "ComplexParameter", "WirtingerGradient",
    "WirtingerSpectralFilter", "spectral_mix_with_filter", "spectral_mix", "spectral_block_mix",
    "pruned_rfft", "DropoutState", "spectral_filter", "rfft_bins", "seq_fft", "hermitian_scale",
    "PhaseAwareSpectralMixing", "MultiScaleSpectralFeatures", "RotaryFrequencyEmbedding", "GatedSpectralUnit",
    "CausalFrequencyMask", "EnhancedSpectralBlock", "ComplexRoPE", "GatedLinearUnit",
    "ComplexRoPESpectralLayer", "FrequencyAttention", "FixedSpectralBlock", "FrequencyConvFunc",
    "causal_spectral_conv", "rfft", "irfft", "FrequencyNativeBlock", "BicameralBlock", "PhaseShift", "SpectralFFN",
    "SpectralLayerNorm", "EMAConfig", "SpectralEMA", "ChunkLM", "vectorized_windows", "ema_scan", "ema_scan_tokens",
    "GradSync", "attach_grad_sync", "all_reduce_grads", "shard_batch", "FixedSpectralLM", "LMConfig", "StreamStates",
    "LayerStream", "stream_taps", "init_layer_states", "update_backbone_chunk", "generate_chunked",
    "PhaseClockHead", "PhaseClockChunkLM", "generate_phase_targets", "compute_phase_clock_loss", "SegmentationHead",
    "SegmentedChunkLM", "get_word_boundaries", "compute_segmented_loss", "word_targets", "narrow_head",
    "DualHead", "TokenAwareChunkLM", "get_token_ids_fast", "compute_dual_loss", "get_gpt2_tokenizer", "cross_entropy",
    "sample_bytes", "SampleConfig", "generate", "ByteSpectralEmbedding", "ByteSpectralEncoder", "SpectralLanguageModel",
    "byte_features", "TrainConfig", "conv_freq_bins", "jpeg_cutoff",
    "curriculum_cutoff", "adaptive_cutoff", "plateau_cutoff", "sawtooth_lr", "lr_stage_params", "make_val_starts",
    "sample_windows", "find_snippets", "load_corpus_as_u8", "eval_loss", "parroting_picks", "parroting_score",
    "save_checkpoint", "verify_checkpoint", "load_checkpoint", "checkpoint_state", "config_from_checkpoint",
    "load_state_flexible", "SparseSpectralTensor", "MemoryManager", "sst", "zeros_sst", "randn_sst", "sparsify_topk",
    "sparse_scatter", "fftn", "ifftn", "spectral_normalize", "spectral_activation", "spectral_pool", "FrequencyMatMul",
    "FrequencyTransformerLayer", "ComplexSemanticEmbedding", "frequency_relu", "frequency_layernorm", "frequency_attention",
    "bin_contract", "OptimizedFrequencyOps", "ProductionFrequencyLinear", "ProductionFrequencyOps",
    "OptimizedSparseSpectralTensor", "polar_range", "polar_quantize", "polar_dequantize", "log8_encode", "log8_decode",
    "log8_encode_complex", "log8_decode_complex", "PolarQuantizer", "ConvolutionTheoremMatMul", "WirtingerAutograd",
    "FrequencyLinearLayer", "LogarithmicQuantizer", "frequency_linear", "frequency_conv1d", "FFTConverter",
    "rowfft_supported", "row_fft_raw", "row_fft", "row_ifft",
]
__version__ = "0.2.0"
