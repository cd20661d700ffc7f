"""Mirror of the offline half of `fft_tensor.llamaizer` (reference fft_tensor/llamaizer.py:24-182): FFTConverter with
convert_linear_to_frequency, convert_model and save_fft_model.  Names, arguments and defaults are the reference's.  The hub
loaders (FFTLlama, FFTGPT, FFTBERT, load_in_fft, the command line) need a model hub and are not mirrored; neither are the
prints."""
import json
from pathlib import Path
from typing import Optional

import torch
import torch.nn as nn

from .zero_materialize import FrequencyLinearLayer


class FFTConverter:
    @staticmethod
    def convert_linear_to_frequency(linear: nn.Linear, sparsity: float = 0.01, learn_phase: bool = True,
                                    quantize: bool = True) -> FrequencyLinearLayer:
        """A FrequencyLinearLayer whose weight is fft(linear.weight, dim=-1) with all but the k = int(in_features *
        sparsity) largest bins of each row zeroed (the reference's per-row mask loop is one scatter), and linear's bias.
        `quantize` is accepted and, as in the reference (where it is a TODO), changes nothing: the weight stays
        complex64.  LogarithmicQuantizer.compress_sparse_freq is the codec it names."""
        in_features = linear.in_features
        out_features = linear.out_features
        has_bias = linear.bias is not None
        freq_linear = FrequencyLinearLayer(in_features, out_features, sparsity=sparsity, bias=has_bias,
                                           learn_phase=learn_phase)
        with torch.no_grad():
            weight_freq = torch.fft.fft(linear.weight.data, dim=-1)
            k = int(in_features * sparsity)
            _, topk_indices = torch.topk(torch.abs(weight_freq), k, dim=-1)
            mask = torch.zeros_like(weight_freq, dtype=torch.bool).scatter_(1, topk_indices, True)
            sparse_freq = weight_freq * mask
            if learn_phase:
                freq_linear.weight_freq.data = sparse_freq
            else:
                freq_linear.weight_magnitude.data = torch.abs(sparse_freq)
                freq_linear.weight_phase.data = torch.angle(sparse_freq)
            if has_bias:
                freq_linear.bias.data = linear.bias.data
        return freq_linear

    @staticmethod
    def convert_model(model: nn.Module, sparsity: float = 0.01, learn_phase: bool = True, quantize: bool = True,
                      skip_layers: Optional[list] = None) -> nn.Module:
        """Replaces, in place and recursively, every nn.Linear child whose name contains none of `skip_layers` (default
        ['embed', 'lm_head', 'head']) by its conversion; returns `model`.  (The reference also prints each layer's
        compress_ratio, which fails there for learn_phase=False; nothing is printed here.)"""
        if skip_layers is None:
            skip_layers = ['embed', 'lm_head', 'head']

        def should_skip(name: str) -> bool:
            return any(pattern in name for pattern in skip_layers)

        for name, module in model.named_children():
            if isinstance(module, nn.Linear) and not should_skip(name):
                setattr(model, name, FFTConverter.convert_linear_to_frequency(module, sparsity, learn_phase, quantize))
            elif len(list(module.children())) > 0:
                FFTConverter.convert_model(module, sparsity, learn_phase, quantize, skip_layers)
        return model

    @staticmethod
    def save_fft_model(model: nn.Module, path: str):
        """Writes `path`/weights.fft (torch.save of {layer name: {weight_freq, bias, in_features, out_features,
        sparsity}} over the model's FrequencyLinearLayers) and `path`/config.json ({num_layers, compression}), as the
        reference does: layers need learn_phase=True, and a model without such layers fails on the mean."""
        path = Path(path)
        path.mkdir(parents=True, exist_ok=True)
        freq_layers = {}
        for name, module in model.named_modules():
            if isinstance(module, FrequencyLinearLayer):
                freq_layers[name] = {
                    'weight_freq': module.weight_freq.data,
                    'bias': module.bias.data if module.bias is not None else None,
                    'in_features': module.in_features,
                    'out_features': module.out_features,
                    'sparsity': module.sparsity,
                }
        torch.save(freq_layers, path / 'weights.fft')
        config = {
            'num_layers': len(freq_layers),
            'compression': sum(
                layer['in_features'] * layer['out_features'] / torch.count_nonzero(layer['weight_freq']).item()
                for layer in freq_layers.values()
            ) / len(freq_layers),
        }
        with open(path / 'config.json', 'w') as f:
            json.dump(config, f, indent=2)
