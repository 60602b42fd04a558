"""MI355X-native DeSTA2.5-Audio model: host side of the hot path.

Mirrors the reference's model surface (desta/models/modeling_desta25.py): `DeSTA25Config` (:633-694),
`DeSTA25AudioModel.forward / state_dict / load_state_dict / from_pretrained` (:698-1050, :1284-1354,
:1723-1747), `WhisperPerception.forward_whisper` (:544-608) and `QformerConnector` (:126-205) — same
names, argument meaning, error behaviour and checkpoint keys — but every FLOP runs in hand-written HIP
kernels behind the C ABI (`desta._hip`).  There is no autograd graph and no tracing compiler: forward
saves the activations the hand-written backward needs into pre-allocated HBM buffers, `backward()`
walks the layers in reverse calling the backward kernels, gradients land in the flat fp32 arena that
the fused Adafactor and the RCCL all-reduce consume.

Precision policy (== HF autocast(bf16) of the reference, hazard H11): GEMM operands bf16 with fp32
accumulation; LayerNorm / RMSNorm / softmax / loss statistics fp32; the LLM residual stream is bf16 (its
weights are loaded in bf16, modeling_desta25.py:715); the Whisper and Q-Former residual streams are fp32
(fp32 weights under autocast: LayerNorm returns fp32 and `fp32 + bf16` promotes, so the reference never
rounds them — with a bf16 Whisper stream the tap error grew with depth, 0.7e-2 -> 1.2e-2 at layer 31
against 0.55e-2 flat for the reference's own policy, tests/test_gpu_model.py::test_deep_*); all trainable
parameters / gradients / optimizer state fp32.
"""
from __future__ import annotations

import json
import logging
import math
import numbers
import os
from collections import OrderedDict
from dataclasses import dataclass, field, asdict
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from .. import _hip as H
from ..optim import ParamArena

BF16, F32 = torch.bfloat16, torch.float32
ENC = "perception.whisper.model.encoder."
CON = "perception.connector."
LLM = "llm_model."

TAP_LAYERS = {  # modeling_desta25.py:134-145 (keyed on the hub name; we key on the name suffix / depth)
    "whisper-tiny": [0, 1, 2, 3], "whisper-small": [2, 5, 8, 11], "whisper-medium": [5, 11, 17, 23],
    "whisper-large-v3": [7, 15, 23, 31], "whisper-large-v3-turbo": [7, 15, 23, 31],
}
_TAPS_BY_DEPTH = {4: [0, 1, 2, 3], 12: [2, 5, 8, 11], 24: [5, 11, 17, 23], 32: [7, 15, 23, 31]}


def _r64(n: int) -> int:
    return (n + 63) // 64 * 64


_M64 = 0xFFFFFFFFFFFFFFFF


def _splitmix64(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def site_seed(seed_base: int, domain: int, layer: int, site: int) -> int:
    """64-bit seed of ONE dropout site of one forward: splitmix64 over (per-forward base, domain, layer, site).  The device RNG
    (csrc/common.h `desta_rng32`) folds a seed into a 32-bit offset + a 32-bit key; hashing on the host means no two sites /
    forwards / ranks are related by a small additive step (packed bit fields made step t + 60 a shifted copy of step t)."""
    return _splitmix64(_splitmix64(seed_base ^ (domain << 56)) + ((layer & 0xFFFFFF) << 8) + (site & 0xFF))


@dataclass
class EncoderConfig:
    num_mel_bins: int = 128
    d_model: int = 1280
    encoder_layers: int = 32
    encoder_attention_heads: int = 20
    encoder_ffn_dim: int = 5120
    max_source_positions: int = 1500
    # Whisper DECODER (only the ASR leg of generate() uses it, modeling_desta25.py:1580-1590); defaults = whisper-large-v3
    decoder_layers: int = 32
    decoder_attention_heads: int = 20
    decoder_ffn_dim: int = 5120
    vocab_size: int = 51866
    max_target_positions: int = 448


@dataclass
class LLMConfig:
    model_type: str = "llama"
    hidden_size: int = 4096
    num_hidden_layers: int = 32
    num_attention_heads: int = 32
    num_key_value_heads: int = 8
    head_dim: int = 128
    intermediate_size: int = 14336
    vocab_size: int = 128256
    rms_norm_eps: float = 1e-5
    rope_theta: float = 500000.0
    rope_scaling: Optional[dict] = None          # {"rope_type":"llama3","factor":8,"low_freq_factor":1,...} or None
    tie_word_embeddings: bool = False
    eos_token_id: Optional[List[int]] = None     # generation stops on any of these (HF generation_config semantics)
    attention_bias: bool = False                 # q_proj / k_proj / v_proj carry a bias (Qwen2 / Qwen2.5: always; else config.json's flag)

    @property
    def qk_norm(self) -> bool:
        return self.model_type == "qwen3"


def check_llm_bias_tensors(c: LLMConfig, names) -> None:
    """Every `*.bias` tensor of the decoder checkpoint has to be one the kernels add: the q|k|v projection biases of an
    `attention_bias` model (TF:models/qwen2/modeling_qwen2.py attention), added by the rotary kernels.  Anything else (Llama's
    `attention_bias` also puts one on o_proj, `mlp_bias` on gate / up / down) raises by name here, at load, instead of being
    dropped silently; so does a checkpoint that lacks a bias its config promises."""
    used = set()
    if c.attention_bias:
        if c.qk_norm:
            raise NotImplementedError(f"attention_bias together with the q/k-norm of model_type '{c.model_type}' is not implemented")
        used = {f"{LLM}model.layers.{i}.self_attn.{m}_proj.bias" for i in range(c.num_hidden_layers) for m in "qkv"}
    if names is None:
        return
    names = set(names)
    for n in sorted(names):
        if n.startswith(LLM) and n.endswith(".bias") and n not in used:
            why = ("o_proj.bias (Llama-style attention_bias)" if n.endswith("o_proj.bias") else
                   "mlp_bias" if ".mlp." in n else
                   "a q|k|v bias without attention_bias in config.json" if n.endswith(("q_proj.bias", "k_proj.bias", "v_proj.bias")) else "an unused bias")
            raise NotImplementedError(f"decoder tensor '{n[len(LLM):]}' is not implemented: {why}; only q_proj / k_proj / v_proj biases are added")
    missing = sorted(used - names)
    if missing:
        raise KeyError(f"attention_bias is set but the checkpoint has no '{missing[0][len(LLM):]}'")


def _read_hf_config(path_or_id: str) -> dict:
    cfg = os.path.join(path_or_id, "config.json")
    if not os.path.isfile(cfg):
        raise FileNotFoundError(
            f"'{path_or_id}' is not a local model directory with a config.json (no hub access here); "
            "pass a local path or explicit llm_config / encoder_config")
    with open(cfg) as f:
        return json.load(f)


class DeSTA25Config:
    """Same fields as the reference's `DeSTA25Config` (modeling_desta25.py:636-694).  `llm_model_id` /
    `encoder_model_id` are local HF model directories (or names, when `llm_config` / `encoder_config`
    are given explicitly — offline there is no hub to resolve names against)."""
    model_type = "desta25"

    def __init__(self, llm_model_id="DeSTA-ntu/Llama-3.1-8B-Instruct", encoder_model_id="openai/whisper-large-v3",
                 connector_mode="qformer_1", qformer_num_hidden_layers=2, prompt_size=64, use_lora=False,
                 audio_locator="<|AUDIO|>", placeholder_token="<|reserved_special_token_87|>",
                 llm_config: Optional[dict] = None, encoder_config: Optional[dict] = None,
                 qformer_intermediate_size: int = 3072, target_layer_ids: Optional[List[int]] = None,
                 qformer_dropout: float = 0.1, orca_enabled=False, orca_use_all_layers=False, orca_local_enabled=True,
                 orca_global_cross_attn=False, orca_deep_injection_enabled=True, orca_audio_position_scale=2.5,
                 orca_global_num_tokens=4, orca_local_downsample=4, orca_local_kernel_size=5, orca_gate_init=0.1,
                 orca_ortho_weight_global=0.01, orca_ortho_diversity_weight=0.01, orca_ortho_weight_qformer_local=0.01,
                 orca_align_weight_local=0.05, **kwargs):
        if connector_mode not in ("qformer_1", "orca_hybrid"):
            raise NotImplementedError(f"mode {connector_mode} not implemented")        # modeling_desta25.py:627
        if connector_mode == "qformer_1" and orca_enabled:
            raise NotImplementedError("orca_enabled with connector_mode 'qformer_1' (the Q-Former auxiliary losses, modeling_desta25.py:846-930) "
                                      "is not implemented")
        # ORCA hybrid: connector, deep injection, auxiliary losses — forward, backward and generation run on the device
        # and are pinned to the reference's goldens.  Field names and defaults: :645-692.
        self.orca_enabled = bool(orca_enabled) or connector_mode == "orca_hybrid"
        self.orca_use_all_layers, self.orca_local_enabled = bool(orca_use_all_layers), bool(orca_local_enabled)
        self.orca_global_cross_attn, self.orca_deep_injection_enabled = bool(orca_global_cross_attn), bool(orca_deep_injection_enabled)
        self.orca_audio_position_scale, self.orca_global_num_tokens = float(orca_audio_position_scale), int(orca_global_num_tokens)
        self.orca_local_downsample, self.orca_local_kernel_size = int(orca_local_downsample), int(orca_local_kernel_size)
        self.orca_gate_init, self.orca_ortho_weight_global = float(orca_gate_init), float(orca_ortho_weight_global)
        self.orca_ortho_diversity_weight, self.orca_ortho_weight_qformer_local = float(orca_ortho_diversity_weight), float(orca_ortho_weight_qformer_local)
        self.orca_align_weight_local = float(orca_align_weight_local)
        # use_lora: peft.LoraConfig(r=16, lora_alpha=16, lora_dropout=0.1, target_modules=[q_proj, k_proj, v_proj]) on the
        # decoder (modeling_desta25.py:720-729); the three constants are fixed there, kept as fields for tests
        self.lora_r, self.lora_alpha = int(kwargs.pop("lora_r", 16)), float(kwargs.pop("lora_alpha", 16))
        self.lora_dropout = float(kwargs.pop("lora_dropout", 0.1))
        self.llm_model_id, self.encoder_model_id = llm_model_id, encoder_model_id
        self.connector_mode, self.qformer_num_hidden_layers, self.prompt_size = connector_mode, qformer_num_hidden_layers, prompt_size
        self.use_lora, self.audio_locator, self.placeholder_token = bool(use_lora), audio_locator, placeholder_token
        self.qformer_intermediate_size = qformer_intermediate_size   # BertConfig() default (never overridden, :156-162)
        # BertConfig() defaults hidden_dropout_prob = attention_probs_dropout_prob = 0.1 are never overridden
        # either (hazard H3): active in training mode, own counter-based RNG (not torch's Philox stream)
        self.qformer_dropout = float(qformer_dropout)
        lc = dict(llm_config) if llm_config is not None else _read_hf_config(llm_model_id)
        ec = dict(encoder_config) if encoder_config is not None else _read_hf_config(encoder_model_id)
        self.llm_config = self._llm_from_dict(lc)
        self.encoder_config = EncoderConfig(**{k: ec[k] for k in asdict(EncoderConfig()) if k in ec})
        if target_layer_ids is not None:
            self.target_layer_ids = list(target_layer_ids)
        else:
            key = os.path.basename(os.path.normpath(encoder_model_id))
            if key in TAP_LAYERS:
                self.target_layer_ids = list(TAP_LAYERS[key])
            elif self.encoder_config.encoder_layers in _TAPS_BY_DEPTH:
                self.target_layer_ids = list(_TAPS_BY_DEPTH[self.encoder_config.encoder_layers])
            else:
                raise NotImplementedError(f"model_id {encoder_model_id} not implemented")
        if connector_mode == "orca_hybrid" and self.orca_use_all_layers and target_layer_ids is None:
            self.target_layer_ids = list(range(self.encoder_config.encoder_layers))       # ORCAHybridConnector.__init__ (:221-224)
        self.info = "Ｄｅｓｔａ２。５ Ａｕｄｉｏ"
        self.extra = dict(kwargs)

    def align_orca_layers(self, n_layers: int) -> bool:
        """A checkpoint whose `global_layer_weights` is [K, n_layers] decides how many encoder layers the ORCA connector taps
        (modeling_desta25.py:1311-1345: a model trained with `orca_use_all_layers` loads into a default-configured one).  n_layers = encoder
        depth -> every layer; any other count -> the first n_layers (the reference names that fallback and then rebuilds its connector
        from the unchanged config, which cannot load; here the fallback is what it says).  -> True when the config changed."""
        if self.connector_mode != "orca_hybrid" or n_layers == len(self.target_layer_ids):
            return False
        self.orca_use_all_layers = n_layers == self.encoder_config.encoder_layers
        self.target_layer_ids = list(range(n_layers))
        return True

    @property
    def audio_tokens(self) -> int:
        """Placeholder tokens one audio clip occupies in the text stream: `prompt_size`, or the global tokens of the ORCA hybrid
        (modeling_desta25.py:1574-1578; the local tokens never enter the sequence)."""
        return self.orca_global_num_tokens if self.connector_mode == "orca_hybrid" else self.prompt_size

    @staticmethod
    def _llm_from_dict(c: dict) -> LLMConfig:
        heads = c.get("num_attention_heads", 32)
        rp = c.get("rope_parameters") or {}
        scaling = c.get("rope_scaling") or ({k: v for k, v in rp.items() if k != "rope_theta"} if rp.get("rope_type", "default") != "default" else None)
        if scaling is not None and scaling.get("rope_type", scaling.get("type", "default")) in ("default", None):
            scaling = None
        # biases and masks no kernel here implements: named at load, never dropped (the tensors themselves: `check_llm_bias_tensors`)
        if c.get("mlp_bias"):
            raise NotImplementedError("mlp_bias: true (biases on gate_proj / up_proj / down_proj) is not implemented")
        if c.get("use_sliding_window"):
            raise NotImplementedError("use_sliding_window: true (sliding-window attention) is not implemented")
        return LLMConfig(
            attention_bias=c.get("model_type", "llama") == "qwen2" or bool(c.get("attention_bias", False)),
            model_type=c.get("model_type", "llama"), hidden_size=c["hidden_size"], num_hidden_layers=c["num_hidden_layers"],
            num_attention_heads=heads, num_key_value_heads=c.get("num_key_value_heads", heads),
            head_dim=c.get("head_dim") or c["hidden_size"] // heads, intermediate_size=c["intermediate_size"],
            vocab_size=c["vocab_size"], rms_norm_eps=c.get("rms_norm_eps", 1e-5),
            rope_theta=float(c.get("rope_theta", rp.get("rope_theta", 10000.0))), rope_scaling=scaling,
            tie_word_embeddings=bool(c.get("tie_word_embeddings", False)),
            eos_token_id=(None if c.get("eos_token_id") is None else
                          [int(t) for t in (c["eos_token_id"] if isinstance(c["eos_token_id"], (list, tuple)) else [c["eos_token_id"]])]))

    def to_dict(self) -> dict:
        return {"model_type": self.model_type, "llm_model_id": self.llm_model_id, "encoder_model_id": self.encoder_model_id,
                "connector_mode": self.connector_mode, "qformer_num_hidden_layers": self.qformer_num_hidden_layers,
                "prompt_size": self.prompt_size, "use_lora": self.use_lora, "audio_locator": self.audio_locator,
                "placeholder_token": self.placeholder_token, "orca_enabled": self.orca_enabled,
                **{k: getattr(self, k) for k in ("orca_use_all_layers", "orca_local_enabled", "orca_global_cross_attn", "orca_deep_injection_enabled",
                                                 "orca_audio_position_scale", "orca_global_num_tokens", "orca_local_downsample", "orca_local_kernel_size",
                                                 "orca_gate_init", "orca_ortho_weight_global", "orca_ortho_diversity_weight",
                                                 "orca_ortho_weight_qformer_local", "orca_align_weight_local")},
                "qformer_intermediate_size": self.qformer_intermediate_size, "target_layer_ids": self.target_layer_ids,
                "qformer_dropout": self.qformer_dropout, "lora_r": self.lora_r, "lora_alpha": self.lora_alpha, "lora_dropout": self.lora_dropout,
                "llm_config": asdict(self.llm_config), "encoder_config": asdict(self.encoder_config), "info": self.info}

    def save_pretrained(self, path: str) -> None:
        os.makedirs(path, exist_ok=True)
        with open(os.path.join(path, "config.json"), "w") as f:
            json.dump(self.to_dict(), f, indent=2)

    @classmethod
    def from_pretrained(cls, path: str, **kwargs) -> "DeSTA25Config":
        d = _read_hf_config(path)
        d.pop("model_type", None)
        d.pop("info", None)
        d.update(kwargs)
        return cls(**d)


def connector_param_shapes(cfg: DeSTA25Config) -> "OrderedDict[str, Tuple[int, ...]]":
    """Trainable tensors with the reference's state-dict names, in ARENA order:
    query/key/value weights (and biases) of every attention block are adjacent so that the fused
    QKV / KV projection GEMMs read them as one [3d, d] / [2d, d] operand."""
    orca = cfg.connector_mode == "orca_hybrid"
    d, K, nt = cfg.encoder_config.d_model, (cfg.orca_global_num_tokens if orca else cfg.prompt_size), len(cfg.target_layer_ids)
    inter, h = cfg.qformer_intermediate_size, cfg.llm_config.hidden_size
    s: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    n_prompts, n_weights, n_qf, n_proj = (("global_queries.", "global_layer_weights", "global_qformer.layer.", "global_proj.") if orca
                                          else ("layer_prompts.", "layer_weights", "qformer.layer.", "proj."))
    for j in range(nt):
        s[f"{CON}{n_prompts}{j}"] = (1, K, d)
    s[f"{CON}{n_weights}"] = (K, nt)
    for i in range(cfg.qformer_num_hidden_layers):
        p = f"{CON}{n_qf}{i}."
        for blk in ("attention", "crossattention"):
            for lin in ("query", "key", "value"):
                s[f"{p}{blk}.self.{lin}.weight"] = (d, d)
            for lin in ("query", "key", "value"):
                s[f"{p}{blk}.self.{lin}.bias"] = (d,)
            s[f"{p}{blk}.output.dense.weight"] = (d, d)
            s[f"{p}{blk}.output.dense.bias"] = (d,)
            s[f"{p}{blk}.output.LayerNorm.weight"] = (d,)
            s[f"{p}{blk}.output.LayerNorm.bias"] = (d,)
        s[p + "intermediate.dense.weight"] = (inter, d)
        s[p + "intermediate.dense.bias"] = (inter,)
        s[p + "output.dense.weight"] = (d, inter)
        s[p + "output.dense.bias"] = (d,)
        s[p + "output.LayerNorm.weight"] = (d,)
        s[p + "output.LayerNorm.bias"] = (d,)
    s[CON + n_proj + "0.weight"] = (d,)
    s[CON + n_proj + "0.bias"] = (d,)
    s[CON + n_proj + "1.weight"] = (h, d)
    s[CON + n_proj + "1.bias"] = (h,)
    if orca:
        # local branch (modeling_desta25.py:266-287) and the gated cross-attention of every decoder layer (:359-393, :1084-1098)
        k = cfg.orca_local_kernel_size
        if cfg.orca_local_enabled:
            s[CON + "local_layer_weights"] = (nt,)
            s[CON + "local_proj_in.weight"] = (h, d)
            s[CON + "local_proj_in.bias"] = (h,)
            s[CON + "local_conv.weight"] = (h, h, k)
            s[CON + "local_conv.bias"] = (h,)
            s[CON + "local_ln.weight"] = (h,)
            s[CON + "local_ln.bias"] = (h,)
        if cfg.orca_deep_injection_enabled:
            for l in range(cfg.llm_config.num_hidden_layers):
                q = f"orca_cross_attns.{l}."
                s[q + "cross_attn.in_proj_weight"] = (3 * h, h)
                s[q + "cross_attn.in_proj_bias"] = (3 * h,)
                s[q + "cross_attn.out_proj.weight"] = (h, h)
                s[q + "cross_attn.out_proj.bias"] = (h,)
                s[q + "gate_proj.0.weight"] = (h // 4, h)
                s[q + "gate_proj.0.bias"] = (h // 4,)
                s[q + "gate_proj.2.weight"] = (1, h // 4)
                s[q + "gate_proj.2.bias"] = (1,)
                s[q + "ln.weight"] = (h,)
                s[q + "ln.bias"] = (h,)
    return s


LORA_TARGETS = ("q", "k", "v")


def lora_param_shapes(cfg: DeSTA25Config) -> "OrderedDict[str, Tuple[int, ...]]":
    """LoRA adapters of the decoder's q/k/v projections under peft's names (`get_peft_model(...).base_model.model`,
    modeling_desta25.py:729), in ARENA order: per layer the three A matrices [r, hidden] adjacent (one [3r, hidden] operand),
    then the three B matrices [out, r] adjacent (one [(Hq + 2 Hkv) hd, r] operand)."""
    s: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    if not cfg.use_lora:
        return s
    c, r = cfg.llm_config, cfg.lora_r
    outs = {"q": c.num_attention_heads * c.head_dim, "k": c.num_key_value_heads * c.head_dim, "v": c.num_key_value_heads * c.head_dim}
    assert (r * c.hidden_size) % 64 == 0 and all((o * r) % 64 == 0 for o in outs.values()) and 3 * r <= 64, "LoRA rank / widths vs arena alignment"
    for i in range(c.num_hidden_layers):
        p = f"{LLM}model.layers.{i}.self_attn."
        for m in LORA_TARGETS:
            s[f"{p}{m}_proj.lora_A.default.weight"] = (r, c.hidden_size)
        for m in LORA_TARGETS:
            s[f"{p}{m}_proj.lora_B.default.weight"] = (outs[m], r)
    return s


def reference_parameter_names(cfg: DeSTA25Config) -> List[str]:
    """Trainable tensors in the REFERENCE's `named_parameters()` order (registration order of
    QformerConnector.__init__, modeling_desta25.py:148-168, and of BertLayer; with `use_lora` the adapters of `llm_model`,
    which is registered before `perception`, come first): the order HF Trainer uses to number parameters inside `optimizer.pt`."""
    names = []
    if getattr(cfg, "use_lora", False):
        names += [f"{LLM}model.layers.{i}.self_attn.{m}_proj.lora_{ab}.default.weight"
                  for i in range(cfg.llm_config.num_hidden_layers) for m in LORA_TARGETS for ab in "AB"]
    orca = getattr(cfg, "connector_mode", "qformer_1") == "orca_hybrid"
    n_prompts, n_weights, n_qf, n_proj = (("global_queries.", "global_layer_weights", "global_qformer.layer.", "global_proj.") if orca
                                          else ("layer_prompts.", "layer_weights", "qformer.layer.", "proj."))
    names += [f"{CON}{n_prompts}{j}" for j in range(len(cfg.target_layer_ids))] + [f"{CON}{n_weights}"]
    for i in range(cfg.qformer_num_hidden_layers):
        p = f"{CON}{n_qf}{i}."
        for blk in ("attention", "crossattention"):
            for lin in ("self.query", "self.key", "self.value", "output.dense", "output.LayerNorm"):
                names += [f"{p}{blk}.{lin}.weight", f"{p}{blk}.{lin}.bias"]
        for lin in ("intermediate.dense", "output.dense", "output.LayerNorm"):
            names += [f"{p}{lin}.weight", f"{p}{lin}.bias"]
    names += [CON + n_proj + "0.weight", CON + n_proj + "0.bias", CON + n_proj + "1.weight", CON + n_proj + "1.bias"]
    if orca:
        # ORCAHybridConnector.__init__ order (:266-287), then `orca_cross_attns` (registered after `perception`, :1084)
        if cfg.orca_local_enabled:
            names += [CON + "local_layer_weights", CON + "local_proj_in.weight", CON + "local_proj_in.bias", CON + "local_conv.weight",
                      CON + "local_conv.bias", CON + "local_ln.weight", CON + "local_ln.bias"]
        if cfg.orca_deep_injection_enabled:
            for l in range(cfg.llm_config.num_hidden_layers):
                q = f"orca_cross_attns.{l}."
                names += [q + "cross_attn.in_proj_weight", q + "cross_attn.in_proj_bias", q + "cross_attn.out_proj.weight", q + "cross_attn.out_proj.bias",
                          q + "gate_proj.0.weight", q + "gate_proj.0.bias", q + "gate_proj.2.weight", q + "gate_proj.2.bias", q + "ln.weight", q + "ln.bias"]
    return names


def rope_inv_freq(c: LLMConfig) -> torch.Tensor:
    """Default / llama3-scaled inverse frequencies (TF:modeling_rope_utils.py, `_compute_llama3_parameters`)."""
    dim = c.head_dim
    inv = 1.0 / (c.rope_theta ** (torch.arange(0, dim, 2, dtype=torch.float64) / dim))
    sc = c.rope_scaling
    if sc is not None and sc.get("rope_type", sc.get("type")) == "llama3":
        factor, lo, hi = sc["factor"], sc["low_freq_factor"], sc["high_freq_factor"]
        old = sc["original_max_position_embeddings"]
        wl = 2 * math.pi / inv
        inv_l = torch.where(wl > old / lo, inv / factor, inv)
        smooth = (old / wl - lo) / (hi - lo)
        sm = (1 - smooth) * inv_l / factor + smooth * inv_l
        med = ~(wl < old / hi) & ~(wl > old / lo)
        inv = torch.where(med, sm, inv_l)
    elif sc is not None:
        raise NotImplementedError(f"rope scaling {sc} not implemented")
    return inv.float()


# HF 5.15 global defaults of the settings the HIP decode loop honours (TF:generation/configuration_utils.py:609-641; min_p has none)
_HF_GEN_DEFAULTS = {"do_sample": False, "temperature": 1.0, "top_k": 50, "top_p": 1.0, "min_p": None, "repetition_penalty": 1.0}
# settings the HIP decode loop cannot honour, with the value that turns each of them off in HF
_HF_GEN_UNSUPPORTED = {"num_beams": 1, "typical_p": 1.0, "epsilon_cutoff": 0.0, "eta_cutoff": 0.0, "top_h": None,
                       "no_repeat_ngram_size": 0, "bad_words_ids": None, "suppress_tokens": None}


# HF's banning processors, honoured by `desta_logit_constraints_bf16` where a caller opts in (`constraints=True` below)
_HF_GEN_CONSTRAINTS = ("no_repeat_ngram_size", "bad_words_ids", "suppress_tokens", "begin_suppress_tokens", "min_new_tokens")
# HF's truncation warpers behind min-p, honoured by `desta_sample_truncated_rows_bf16` where a caller opts in (`truncation=True`)
_HF_GEN_TRUNCATION = ("typical_p", "epsilon_cutoff", "eta_cutoff")


def resolve_generation_kwargs(llm_generation_config: dict, *, constraints: bool = False, truncation: bool = False, **explicit) -> dict:
    """The sampling settings HF's `generate` would use (TF:generation/utils.py:1806-1808): an explicit argument, else the
    checkpoint's `generation_config.json`, else HF's global default (so top_k = 50 unless someone says otherwise).  `None`
    counts as unset.  Keys other than the sampling settings (max_new_tokens, seed, ...) pass through.  Raises
    NotImplementedError for any setting this path cannot honour that is set away from HF's default (beam search, typical_p,
    epsilon / eta cutoffs, top_h, no_repeat_ngram_size, bad_words_ids, suppress_tokens).
    constraints=True: no_repeat_ngram_size, bad_words_ids, suppress_tokens, begin_suppress_tokens and min_new_tokens are
    resolved as well (explicit, else the file's, else None = off; 0 and [] count as off) and returned for `generate` instead of
    raising; the other settings of that list still raise.
    truncation=True: typical_p, epsilon_cutoff and eta_cutoff are resolved as well (explicit, else the file's, else None = off;
    typical_p = 1.0 and a cutoff of 0.0 count as off) and returned for `generate` instead of raising.  Beam search and top_h
    raise under every combination."""
    file_cfg = dict(llm_generation_config or {})
    bad = []
    for k, off in _HF_GEN_UNSUPPORTED.items():
        if (constraints and k in _HF_GEN_CONSTRAINTS) or (truncation and k in _HF_GEN_TRUNCATION):
            continue
        v = explicit.get(k) if explicit.get(k) is not None else file_cfg.get(k)
        if v is not None and v != off and v != []:
            bad.append(f"{k}={v!r}")
    if bad:
        raise NotImplementedError(f"generation settings not supported by the HIP decode loop: {', '.join(bad)}")
    out = {k: v for k, v in explicit.items() if k not in _HF_GEN_UNSUPPORTED}
    for k, default in _HF_GEN_DEFAULTS.items():
        v = explicit.get(k)
        out[k] = v if v is not None else (file_cfg[k] if file_cfg.get(k) is not None else default)
    if constraints:
        for k in _HF_GEN_CONSTRAINTS:
            v = explicit.get(k) if explicit.get(k) is not None else file_cfg.get(k)
            out[k] = None if (v is None or v == [] or (v == 0 and not isinstance(v, bool))) else v
    if truncation:
        for k in _HF_GEN_TRUNCATION:
            v = explicit.get(k) if explicit.get(k) is not None else file_cfg.get(k)
            out[k] = None if (v is None or (not isinstance(v, bool) and v == _HF_GEN_UNSUPPORTED[k])) else v
    return out


def check_sampling_args(top_k=None, min_p=None, repetition_penalty=None) -> None:
    """HF's argument checks for the processors behind top_k / min_p / repetition_penalty (TF:generation/logits_process.py
    RepetitionPenaltyLogitsProcessor, TopKLogitsWarper, MinPLogitsWarper); None means off, top_k = 0 too."""
    if repetition_penalty is not None and not (isinstance(repetition_penalty, (int, float)) and repetition_penalty > 0):
        raise ValueError(f"`penalty` has to be a strictly positive float, but is {repetition_penalty}")
    if top_k is not None and (isinstance(top_k, bool) or not isinstance(top_k, int) or top_k < 0):
        raise ValueError(f"`top_k` has to be a strictly positive integer, but is {top_k}")
    if min_p is not None and not (isinstance(min_p, (int, float)) and 0 <= min_p <= 1.0):
        raise ValueError(f"`min_p` has to be a float in the [0, 1] interval, but is {min_p}")


def check_truncation_args(typical_p=None, epsilon_cutoff=None, eta_cutoff=None) -> None:
    """HF's argument checks for TypicalLogitsWarper, EpsilonLogitsWarper and EtaLogitsWarper (TF:generation/logits_process.py),
    with HF's messages; None means off, and so do the values HF's `_get_logits_processor` skips the warper for: typical_p = 1.0,
    epsilon_cutoff = 0.0, eta_cutoff = 0.0."""
    for name, v, off in (("typical_p", typical_p, 1.0), ("epsilon_cutoff", epsilon_cutoff, 0.0), ("eta_cutoff", eta_cutoff, 0.0)):
        real = isinstance(v, numbers.Real) and not isinstance(v, bool)     # HF takes float(v): numpy scalars and ints are fine
        if v is None or (real and v == off):
            continue
        if not real:
            raise ValueError(f"`{name}` has to be a float > 0 and < 1, but is {v}")
        if not (0 < v < 1):
            raise ValueError(f"`{name}` has to be a float > 0 and < 1, but is {float(v)}")      # HF converts first: 2 reads "2.0"


def truncation_kwargs(do_sample: bool, typical_p=None, epsilon_cutoff=None, eta_cutoff=None) -> dict:
    """The keyword arguments `H.sample` / `H.sample_rows` take for steps 7-9 of the chain: empty when every step is off or the
    call does not sample (HF's warpers run under do_sample=True only), so such a call reaches the kernels it always reached."""
    check_truncation_args(typical_p, epsilon_cutoff, eta_cutoff)
    kw = dict(typical_p=1.0 if typical_p is None else float(typical_p), epsilon_cutoff=float(epsilon_cutoff or 0.0),
              eta_cutoff=float(eta_cutoff or 0.0))
    return kw if do_sample and kw != dict(typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0) else {}


def _is_id(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool) and v >= 0


def check_constraint_args(no_repeat_ngram_size=None, bad_words_ids=None, suppress_tokens=None, begin_suppress_tokens=None,
                          min_new_tokens=None, vocab: Optional[int] = None) -> None:
    """HF's argument checks for the banning processors (TF:generation/logits_process.py NoRepeatNGramLogitsProcessor,
    NoBadWordsLogitsProcessor, MinNewTokensLengthLogitsProcessor; SuppressTokens[AtBegin]LogitsProcessor take a list of ids);
    None means off.  vocab (where it is known): every id has to lie below it, since only ids in [0, vocab) can be banned."""
    n = no_repeat_ngram_size
    if n is not None and (isinstance(n, bool) or not isinstance(n, int) or n <= 0):
        raise ValueError(f"`no_repeat_ngram_size` (HF's `ngram_size`) has to be a strictly positive integer, but is {n}")
    if bad_words_ids is not None:
        if not isinstance(bad_words_ids, list) or len(bad_words_ids) == 0:
            raise ValueError(f"`bad_words_ids` has to be a non-empty list, but is {bad_words_ids}.")
        if any(not isinstance(w, list) or len(w) == 0 for w in bad_words_ids):
            raise ValueError(f"`bad_words_ids` has to be a list of non-empty lists, but is {bad_words_ids}.")
        if any(not _is_id(t) for w in bad_words_ids for t in w):
            raise ValueError(f"Each list in `bad_words_ids` has to be a list of positive integers, but is {bad_words_ids}.")
    for name, ids in (("suppress_tokens", suppress_tokens), ("begin_suppress_tokens", begin_suppress_tokens)):
        if ids is not None and (not isinstance(ids, (list, tuple)) or any(not _is_id(t) for t in ids)):
            raise ValueError(f"`{name}` has to be a list of non-negative integers, but is {ids}")
    m = min_new_tokens
    if m is not None and (isinstance(m, bool) or not isinstance(m, int) or m < 0):
        raise ValueError(f"`min_new_tokens` has to be a non-negative integer, but is {m}")
    if vocab is not None:
        for name, ids in (("bad_words_ids", [t for w in bad_words_ids or [] for t in w]), ("suppress_tokens", suppress_tokens or []),
                          ("begin_suppress_tokens", begin_suppress_tokens or [])):
            over = [t for t in ids if t >= vocab]
            if over:
                raise ValueError(f"`{name}` holds token id {over[0]}, the vocabulary has {vocab} tokens")
    n_sup = len(suppress_tokens or [])                                       # they join the word table as one-token words
    if len(bad_words_ids or []) + n_sup > H.CONSTRAINT_MAX_WORDS or sum(len(w) for w in bad_words_ids or []) + n_sup > H.CONSTRAINT_MAX_WORD_IDS:
        raise ValueError(f"`bad_words_ids` and `suppress_tokens` together hold more than {H.CONSTRAINT_MAX_WORDS} words or "
                         f"{H.CONSTRAINT_MAX_WORD_IDS} ids")


def constraint_tables(eos_token_ids=None, no_repeat_ngram_size=None, bad_words_ids=None, suppress_tokens=None,
                      begin_suppress_tokens=None, min_new_tokens=None) -> dict:
    """The host form of a call's constraint tables, as `desta_logit_constraints_bf16` takes them: `[e]` words of an EOS id e
    dropped (NoBadWordsLogitsProcessor.__init__ does that), suppress_tokens appended as one-token words (EOS not filtered there),
    the words flattened to ids + offsets; min_new_tokens off when the call has no EOS."""
    eos = [int(e) for e in (eos_token_ids or [])]
    words = [[int(t) for t in w] for w in (bad_words_ids or []) if not (len(w) == 1 and int(w[0]) in eos)]
    words += [[int(t)] for t in (suppress_tokens or [])]
    off = [0]
    for w in words:
        off.append(off[-1] + len(w))
    begin = [int(t) for t in (begin_suppress_tokens or [])]
    min_new = int(min_new_tokens or 0) if eos else 0
    return dict(no_repeat_ngram=int(no_repeat_ngram_size or 0), word_ids=[t for w in words for t in w], word_off=off, n_words=len(words),
                begin_ids=begin, eos_ids=eos if min_new else [], min_new_tokens=min_new)


class ConstraintPlan:
    """The constraints of one generate() call on the device, built once: the int32 tables of `constraint_tables` and the scalar
    settings.  `active` is False when every rule is off (the loop then runs as without a plan); `apply` is one
    `H.logit_constraints` launch."""

    def __init__(self, device, eos_token_ids=None, no_repeat_ngram_size=None, bad_words_ids=None, suppress_tokens=None,
                 begin_suppress_tokens=None, min_new_tokens=None):
        t = constraint_tables(eos_token_ids, no_repeat_ngram_size, bad_words_ids, suppress_tokens, begin_suppress_tokens, min_new_tokens)

        def dev(ids):
            return torch.tensor(ids, dtype=torch.int32, device=device) if ids else None
        ids = t["word_ids"] + t["begin_ids"] + t["eos_ids"]
        self.kw = dict(no_repeat_ngram=t["no_repeat_ngram"], word_ids=dev(t["word_ids"]), word_off=dev(t["word_off"]) if t["n_words"] else None,
                       n_words=t["n_words"], n_word_ids=len(t["word_ids"]), begin_ids=dev(t["begin_ids"]), n_begin=len(t["begin_ids"]),
                       eos_ids=dev(t["eos_ids"]), n_eos=len(t["eos_ids"]), min_new_tokens=t["min_new_tokens"], id_max=max(ids, default=-1))
        self.active = bool(t["no_repeat_ngram"] or t["n_words"] or t["begin_ids"] or t["min_new_tokens"])

    def apply(self, src, ld_src, dst, ld_dst, batch, width, cols, hist, hist_len, tail=None, step0=0) -> None:
        H.logit_constraints(src, ld_src, dst, ld_dst, batch, width, cols, hist=hist, hist_len=hist_len, tail=tail, step0=step0, **self.kw)


def check_logprobs_arg(n) -> None:
    """`logprobs=` of generate(): None (off) or the number of top alternatives per token, an int in 0..H.TOPK_LOGPROBS_MAX."""
    if n is None:
        return
    if isinstance(n, bool) or not isinstance(n, int) or not 0 <= n <= H.TOPK_LOGPROBS_MAX:
        raise ValueError(f"`logprobs` has to be None or an integer in [0, {H.TOPK_LOGPROBS_MAX}], but is {n!r}")


def check_decode_rows(B: int, guided: bool = False, limit: Optional[int] = None) -> None:
    """A KV-cached decode step streams the weights once for all its rows; its projections take at most H.DECODE_MAX_ROWS of them,
    or the model's `set_decode_rows` ceiling (`limit`).  guided: B counts the unconditional rows of a `guidance_scale` call as well."""
    limit = H.DECODE_MAX_ROWS if limit is None else limit
    if B > limit:
        if guided:
            raise ValueError(f"generate: guidance_scale doubles the rows (one unconditional row per sequence): {B // 2} sequences are {B} rows, "
                             f"the KV-cached decode step takes at most {limit}: split the batch")
        raise ValueError(f"generate: a batch of {B} sequences, the KV-cached decode step takes at most {limit}: split the batch")


def check_decode_rows_arg(n) -> None:
    """`set_decode_rows`: None or H.DECODE_MAX_ROWS (the default ceiling) or an int up to H.DECODE_TALL_MAX_ROWS."""
    if n is None:
        return
    if isinstance(n, bool) or not isinstance(n, int) or not H.DECODE_MAX_ROWS <= n <= H.DECODE_TALL_MAX_ROWS:
        raise ValueError(f"decode_rows must be None or an int in {H.DECODE_MAX_ROWS}..{H.DECODE_TALL_MAX_ROWS}, got {n!r}")


PERCEPTION_SLICE = 64                               # audios per encoder + connector call of generate() above that many (H.DECODE_MAX_ROWS)
TALL_PREFILL_ROWS = 16384                         # rows of one prompt chunk above H.DECODE_MAX_ROWS sequences: a memory bound
TALL_GEMM_ROWS = 8192                               # `tall_rows_to_gemm`: bf16 weight rows from which the tile GEMM takes a tall step's projection
TALL_GEMM_ROWS_ABOVE_128 = 6144                     # ... and from which it does at more than 128 rows


def tall_rows_to_gemm(M: int, weight_rows: int) -> bool:
    """bf16 projections of a step of more than H.DECODE_MAX_ROWS rows that go to `H.gemm` instead of `H.gemm_tall`: a rule of the
    shape alone, from the five Llama-3.1-8B shapes at M = 65, 128, 192, 256 (DESIGN §3 "Decode at batch 65–256").  The tile GEMM
    won gate|up (28672 weight rows) and the lm_head (128256) at every M and q|k|v (6144) at M = 192 and 256; `gemm_tall` won o and
    down (4096) at every M and q|k|v at M = 65 and 128.  The thresholds (TALL_GEMM_ROWS, TALL_GEMM_ROWS_ABOVE_128) sit between
    those shapes."""
    return weight_rows >= TALL_GEMM_ROWS or (weight_rows >= TALL_GEMM_ROWS_ABOVE_128 and M > 128)


def tall_prefill_chunk(B: int) -> Optional[int]:
    """Chunk of the prompt pass of more than H.DECODE_MAX_ROWS sequences where `set_prefill_chunk` names none: the largest multiple
    of 16 positions with B * chunk <= TALL_PREFILL_ROWS rows (B = 65: 240, 128: 128, 256: 64).  A memory rule: the training
    `forward` keeps a save set per layer and prompt row, the lean pass one set of TALL_PREFILL_ROWS rows (about 2.3 GB at
    Llama-3.1-8B's widths); nothing was tuned.  None at or under H.DECODE_MAX_ROWS sequences: nothing changes there."""
    if B <= H.DECODE_MAX_ROWS:
        return None
    return max(PREFILL_CHUNK_MIN, TALL_PREFILL_ROWS // B // 16 * 16)


def check_guidance_arg(g) -> None:
    """`guidance_scale=` of generate(): None (off) or a finite real > 0 (1 is off as well: HF builds no processor at scale 1)."""
    if g is None:
        return
    if isinstance(g, bool) or not isinstance(g, (int, float)) or not (g > 0 and math.isfinite(g)):
        raise ValueError(f"`guidance_scale` has to be None or a finite number > 0, but is {g!r}")


def guidance_negative_messages(messages, audio_locator: str):
    """The negative prompt `generate(guidance_scale=)` derives when none is given: the same chat without its audio.  Every
    conversation of `messages` (one conversation, or a list of them) is copied with each `audio_locator` taken out of every
    `content` (str.replace, nothing else touched) and the `audios` entries dropped; the input is not modified."""
    def strip(conv):
        neg = []
        for m in conv:
            m2 = {k: v for k, v in m.items() if k != "audios"}
            if isinstance(m2.get("content"), str):
                m2["content"] = m2["content"].replace(audio_locator, "")
            neg.append(m2)
        return neg
    if messages and isinstance(messages[0], dict):
        return strip(messages)
    return [strip(conv) for conv in messages]


PREFILL_CHUNK_MIN = 16                              # positions: a 16-row MFMA tile; below it a chunk is launch overhead only


def check_prefill_chunk(n) -> None:
    """`set_prefill_chunk`: None (the training forward as the prompt pass) or an int of at least PREFILL_CHUNK_MIN positions."""
    if n is None:
        return
    if isinstance(n, bool) or not isinstance(n, int) or n < PREFILL_CHUNK_MIN:
        raise ValueError(f"prefill_chunk must be None or an int >= {PREFILL_CHUNK_MIN}, got {n!r}")


SPECULATIVE_MAX = 7                                 # draft tokens per verify step (desta_spec_accept)
SPEC_NGRAM_MAX, SPEC_NGRAM_MIN = 3, 1               # suffix lengths the prompt lookup tries, longest first


def check_speculative_arg(k) -> None:
    """`set_speculative`: None or 0 (off) or the number of draft tokens per verify step, an int in 1..SPECULATIVE_MAX."""
    if k is None:
        return
    if isinstance(k, bool) or not isinstance(k, int) or not 0 <= k <= SPECULATIVE_MAX:
        raise ValueError(f"speculative must be None, 0 or an int in 1..{SPECULATIVE_MAX} draft tokens per step, got {k!r}")


SPECULATIVE_SCOPES = ("greedy", "all")              # which generate() calls `set_speculative` covers


SPECULATIVE_ATTENTIONS = ("forward", "split")       # which kernel a verify step of `set_speculative` attends through


def check_speculative_attention(attention) -> None:
    """`set_speculative(k, attention=...)`: "forward" (the causal forward kernel) or "split" (the split-KV verify kernels)."""
    if attention not in SPECULATIVE_ATTENTIONS:
        raise ValueError(f"speculative attention must be one of {SPECULATIVE_ATTENTIONS}, got {attention!r}")


def check_speculative_scope(scope) -> None:
    """`set_speculative(k, scope=...)`: "greedy" (plain greedy calls only) or "all" (sampling, repetition penalty, logprobs too)."""
    if not isinstance(scope, str) or scope not in SPECULATIVE_SCOPES:
        raise ValueError(f"speculative scope must be one of {SPECULATIVE_SCOPES}, got {scope!r}")


def prefill_chunks(S: int, C: int) -> List[Tuple[int, int]]:
    """Position ranges [c0, c1) of the chunked prompt pass: [0, S) in order, C positions each, a ragged last one."""
    return [(c0, min(c0 + C, S)) for c0 in range(0, S, C)]


@dataclass
class GenerationOutput:
    """modeling_desta25.py:492-496"""
    audios: list
    generated_ids: list
    text: list
    # generate(..., logprobs=n) only, under the model's own distribution (log_softmax of the raw logits); None otherwise
    token_logprobs: Optional[list] = None      # B lists of floats: the row's tokens up to and including its first EOS
    top_logprobs: Optional[list] = None        # per row and token: n tuples (token_id, token string or None, logprob), most likely first
    sum_logprob: Optional[list] = None         # B floats: sum of the row's token_logprobs


@dataclass
class TokenLogprobs:
    """`generate_greedy(logprobs=n)`: the log-probability of every emitted token and the n most likely tokens of its step, under
    log_softmax of the raw logits.  Columns behind a row's EOS hold 0 / -1 / 0."""
    token_logprobs: torch.Tensor       # [B, n_new] fp32
    top_ids: torch.Tensor              # [B, n_new, n] int32, descending probability, lower id first among equals
    top_logprobs: torch.Tensor         # [B, n_new, n] fp32


@dataclass
class ScoreOutput:
    """`score_batch`: log-likelihood of every row's target tokens under the model (targets = labels != -100 after the causal shift)."""
    sum_logprob: torch.Tensor          # [B] fp32: sum of the row's token log-probs
    n_tokens: torch.Tensor             # [B] int64: target tokens of the row
    token_logprobs: list               # B 1-D fp32 tensors, sequence order
    top1_match: torch.Tensor           # [B] int64: target tokens that are the argmax of their logits row
    loss: torch.Tensor                 # the scalar `forward` returns for the same batch (token-mean CE)


@dataclass
class ChoiceScores:
    """`score`: one conversation, ranked answer options."""
    scores: torch.Tensor               # [n_choices] fp32: sum of token log-probs ("sum") or that sum / n_tokens ("mean")
    best: int                          # argmax of `scores`
    token_logprobs: list               # n_choices 1-D fp32 tensors: the choice's tokens, then EOS
    n_tokens: torch.Tensor             # [n_choices] int64


def check_score_args(choices, normalize) -> None:
    if normalize not in ("sum", "mean"):
        raise ValueError(f"`normalize` has to be \"sum\" or \"mean\", but is {normalize!r}")
    if not isinstance(choices, (list, tuple)) or len(choices) == 0:
        raise ValueError("`choices` has to be a non-empty list of strings")
    for c in choices:
        if not isinstance(c, str) or len(c) == 0:
            raise ValueError(f"every choice has to be a non-empty string, got {c!r}")


class _Out:
    """`CausalLMOutputWithPast`-shaped result (`.loss` 0-d fp32 tensor, `.logits` [B,S,V])."""

    def __init__(self, loss, logits):
        self.loss, self.logits = loss, logits

    def __getitem__(self, k):
        return getattr(self, k)


# =========================================================================================== Whisper encoder
class WhisperEncoderHIP:
    """Frozen Whisper encoder, forward only (modeling_desta25.py:551-585; no final layer_norm, H2)."""

    def __init__(self, cfg: DeSTA25Config, w: Dict[str, torch.Tensor], device):
        e = cfg.encoder_config
        self.cfg, self.e, self.dev = cfg, e, device
        self.d, self.L, self.heads, self.ffn, self.T = e.d_model, e.encoder_layers, e.encoder_attention_heads, e.encoder_ffn_dim, e.max_source_positions
        assert self.d // self.heads == 64, "Whisper head_dim is 64 for every released size"
        self.Cp = _r64(e.num_mel_bins)
        dev = device

        def g(name):
            return w[ENC + name].to(dev)
        c1 = g("conv1.weight").float()                                  # [d, C, 3]
        w1 = torch.zeros(self.d, 3, self.Cp, dtype=F32, device=dev)
        w1[:, :, : e.num_mel_bins] = c1.permute(0, 2, 1)
        self.conv1_w = w1.reshape(self.d, 3 * self.Cp).to(BF16).contiguous()
        self.conv1_b = g("conv1.bias").float().contiguous()
        self.conv2_w = g("conv2.weight").float().permute(0, 2, 1).reshape(self.d, 3 * self.d).to(BF16).contiguous()
        self.conv2_b = g("conv2.bias").float().contiguous()
        self.pos = g("embed_positions.weight")[: self.T].float().contiguous()          # fp32: added to the fp32 residual stream
        self.layers = []
        for i in range(self.L):
            p = f"layers.{i}."
            qw, kw, vw = g(p + "self_attn.q_proj.weight"), g(p + "self_attn.k_proj.weight"), g(p + "self_attn.v_proj.weight")
            qb, vb = g(p + "self_attn.q_proj.bias").float(), g(p + "self_attn.v_proj.bias").float()
            self.layers.append(dict(
                ln1_g=g(p + "self_attn_layer_norm.weight").float().contiguous(), ln1_b=g(p + "self_attn_layer_norm.bias").float().contiguous(),
                wqkv=torch.cat([qw, kw, vw], 0).to(BF16).contiguous(),
                bqkv=torch.cat([qb, torch.zeros_like(qb), vb]).contiguous(),           # k_proj has no bias (H6)
                wo=g(p + "self_attn.out_proj.weight").to(BF16).contiguous(), bo=g(p + "self_attn.out_proj.bias").float().contiguous(),
                ln2_g=g(p + "final_layer_norm.weight").float().contiguous(), ln2_b=g(p + "final_layer_norm.bias").float().contiguous(),
                w1=g(p + "fc1.weight").to(BF16).contiguous(), b1=g(p + "fc1.bias").float().contiguous(),
                w2=g(p + "fc2.weight").to(BF16).contiguous(), b2=g(p + "fc2.bias").float().contiguous()))
        self.B = 0

    def _alloc(self, B: int, enc_all: torch.Tensor):
        d, T, dev = self.d, self.T, self.dev
        self.B = B
        self.melrows = torch.zeros(B, 2 * T + 2, self.Cp, dtype=BF16, device=dev)
        self.h1 = torch.zeros(B, 2 * T + 1, d, dtype=BF16, device=dev)          # row 0 of each clip stays 0 (conv2 left pad)
        # residual stream in fp32: ONE buffer, updated in place (see forward)
        self.xr = [torch.empty(B * T, d, dtype=F32, device=dev)]
        self.hb = torch.empty(B * T, d, dtype=BF16, device=dev)
        self.qkv = torch.empty(B * T, 3 * d, dtype=BF16, device=dev)
        self.att = torch.empty(B * T, d, dtype=BF16, device=dev)
        self.ff = torch.empty(B * T, self.ffn, dtype=BF16, device=dev)

    def forward(self, mel: torch.Tensor, enc_all: torch.Tensor) -> None:
        """mel [B, n_mels, 2T] fp32 -> enc_all [taps, B*T, d] bf16 (tapped hidden states)."""
        e, d, T = self.e, self.d, self.T
        B = mel.shape[0]
        if mel.shape[-1] != 2 * T:
            raise ValueError(f"Whisper expects the mel input features to be of length {2 * T}, but found "
                             f"{mel.shape[-1]}. Make sure to pad the input mel features to {2 * T}.")
        if B != self.B:
            self._alloc(B, enc_all)
        M = B * T
        H.mel_to_rows(mel, self.Cp, self.melrows)
        # conv1 (k3,s1,p1) + GELU as a zero-copy im2col GEMM over the padded channel-last rows
        H.gemm(self.melrows, self.conv1_w, self.h1[:, 1:], 2 * T, d, 3 * self.Cp, lda=self.Cp, ldc=d, bias=self.conv1_b,
               act=1, batch=B, stride_a=(2 * T + 2) * self.Cp, stride_c=(2 * T + 1) * d)
        # conv2 (k3,s2,p1) + GELU + positions
        # the fp32 residual stream lives in ONE buffer, updated in place by the out-proj / fc2 epilogues (x += ...: every element is read
        # and written by the same lane): 61 MB that stay in the 256-MB Infinity Cache from layer to layer, where three rotating
        # buffers (184 MB) did not
        x = self.xr[0]
        H.gemm(self.h1, self.conv2_w, x, T, d, 3 * d, lda=2 * d, ldc=d, bias=self.conv2_b, act=1,
               residual=self.pos, ldr=d, stride_r=0, batch=B, stride_a=(2 * T + 1) * d, stride_c=T * d)
        taps = self.cfg.target_layer_ids
        scale = 64 ** -0.5
        for i, ly in enumerate(self.layers):
            H.layernorm_fwd(x, ly["ln1_g"], ly["ln1_b"], 1e-5, y16=self.hb)
            H.gemm(self.hb, ly["wqkv"], self.qkv, M, 3 * d, d, bias=ly["bqkv"])
            ad = H.attn_desc(self.qkv, self.qkv, self.qkv, self.att, None, batch=B, hq=self.heads, hkv=self.heads, sq=T, sk=T,
                             hd=64, scale=scale, q_off=0, k_off=d, v_off=2 * d)
            H.attention_fwd(ad)
            H.gemm(self.att, ly["wo"], x, M, d, d, bias=ly["bo"], residual=x)
            H.layernorm_fwd(x, ly["ln2_g"], ly["ln2_b"], 1e-5, y16=self.hb)
            H.gemm(self.hb, ly["w1"], self.ff, M, self.ffn, d, bias=ly["b1"], act=1)
            H.gemm(self.ff, ly["w2"], x, M, d, self.ffn, bias=ly["b2"], residual=x)
            if i in taps:                                   # the Q-Former's K/V projections read the tapped state as a bf16 operand
                H.cast_bf16(x, enc_all[taps.index(i)], M * d)
        self.last32 = x                                   # output of the last layer, fp32 [B*T, d] (the ASR decoder applies encoder.layer_norm to it)


# =========================================================================================== Whisper decoder (ASR leg of generate)
DEC = "perception.whisper.model.decoder."


class WhisperDecoderHIP:
    """Greedy KV-cached Whisper decoder: the `self.perception.whisper.generate(input_features=..., attention_mask=None,
    max_new_tokens=128)` call of the reference's chat-level `generate` (modeling_desta25.py:1580-1590), which transcribes every clip
    that has speech and no text.  The arithmetic the reference delegates to `WhisperForConditionalGeneration` (TF:models/whisper/
    modeling_whisper.py decoder layers :415-520, generation_whisper.py): pre-LN decoder layers with causal self-attention over a
    cache, cross-attention over the 1500 final encoder states (encoder.layer_norm applied, which the perception taps skip, H2),
    GELU FFN, tied output projection; init tokens [start, detected language, no-timestamps] for a multilingual checkpoint with
    language / task unset, the `suppress_tokens` / `begin_suppress_tokens` lists, greedy until EOS or max_new_tokens.  Every GEMM runs on
    the weight-streaming (decode) kernel, attention on the Sq = 1 flash kernel, bf16 operands with an fp32 residual stream (the
    reference runs this call in fp32).  Returns the NEW tokens (init tokens stripped, finished rows padded with pad_token_id),
    i.e. what the reference's plain-tensor return holds for a clip that ends with EOS inside one 30-s segment.
    Pinned to `WhisperForConditionalGeneration.generate` on a tiny local-config model: tests/test_gpu_generate.py."""

    def __init__(self, cfg: DeSTA25Config, w: Dict[str, torch.Tensor], device, gen_cfg: Optional[dict] = None):
        e = cfg.encoder_config
        self.e, self.dev = e, device
        self.d, self.L, self.heads, self.ffn, self.V, self.Tmax = e.d_model, e.decoder_layers, e.decoder_attention_heads, e.decoder_ffn_dim, e.vocab_size, e.max_target_positions
        assert self.d // self.heads == 64, "Whisper head_dim is 64"
        self.Vp = _r64(self.V)
        dev = device

        def g(name):
            return w[name].to(dev)
        d = self.d
        self.emb32 = g(DEC + "embed_tokens.weight").float().contiguous()
        self.emb16 = torch.zeros(self.Vp, d, dtype=BF16, device=dev)
        self.emb16[: self.V] = self.emb32.to(BF16)                                 # proj_out is tied to embed_tokens
        self.pos32 = g(DEC + "embed_positions.weight").float().contiguous()
        self.ln_post = (g(ENC + "layer_norm.weight").float().contiguous(), g(ENC + "layer_norm.bias").float().contiguous())
        self.ln_f = (g(DEC + "layer_norm.weight").float().contiguous(), g(DEC + "layer_norm.bias").float().contiguous())
        self.layers = []
        for i in range(self.L):
            p = f"{DEC}layers.{i}."
            z = torch.zeros(d, dtype=F32, device=dev)
            self.layers.append(dict(
                ln1=(g(p + "self_attn_layer_norm.weight").float().contiguous(), g(p + "self_attn_layer_norm.bias").float().contiguous()),
                wq=g(p + "self_attn.q_proj.weight").to(BF16).contiguous(), bq=g(p + "self_attn.q_proj.bias").float().contiguous(),
                wkv=torch.cat([g(p + "self_attn.k_proj.weight"), g(p + "self_attn.v_proj.weight")], 0).to(BF16).contiguous(),
                bkv=torch.cat([z, g(p + "self_attn.v_proj.bias").float()]).contiguous(),           # k_proj has no bias
                wo=g(p + "self_attn.out_proj.weight").to(BF16).contiguous(), bo=g(p + "self_attn.out_proj.bias").float().contiguous(),
                ln2=(g(p + "encoder_attn_layer_norm.weight").float().contiguous(), g(p + "encoder_attn_layer_norm.bias").float().contiguous()),
                cwq=g(p + "encoder_attn.q_proj.weight").to(BF16).contiguous(), cbq=g(p + "encoder_attn.q_proj.bias").float().contiguous(),
                cwkv=torch.cat([g(p + "encoder_attn.k_proj.weight"), g(p + "encoder_attn.v_proj.weight")], 0).to(BF16).contiguous(),
                cbkv=torch.cat([z, g(p + "encoder_attn.v_proj.bias").float()]).contiguous(),
                cwo=g(p + "encoder_attn.out_proj.weight").to(BF16).contiguous(), cbo=g(p + "encoder_attn.out_proj.bias").float().contiguous(),
                ln3=(g(p + "final_layer_norm.weight").float().contiguous(), g(p + "final_layer_norm.bias").float().contiguous()),
                w1=g(p + "fc1.weight").to(BF16).contiguous(), b1=g(p + "fc1.bias").float().contiguous(),
                w2=g(p + "fc2.weight").to(BF16).contiguous(), b2=g(p + "fc2.bias").float().contiguous()))
        gc = dict(gen_cfg or {})
        self.start_id = int(gc.get("decoder_start_token_id", 50258))
        eos = gc.get("eos_token_id", 50257)
        self.eos_ids = [int(t) for t in (eos if isinstance(eos, (list, tuple)) else [eos])]
        self.pad_id = int(gc.get("pad_token_id", self.eos_ids[0]))
        self.lang_ids = sorted(int(v) for v in (gc.get("lang_to_id") or {}).values()) if gc.get("is_multilingual", False) else []
        self.no_ts_id = gc.get("no_timestamps_token_id")
        self.suppress = [int(t) for t in (gc.get("suppress_tokens") or [])]
        self.begin_suppress = [int(t) for t in (gc.get("begin_suppress_tokens") or [])]

        def idx(v):
            return torch.tensor(v, dtype=torch.int32, device=dev) if v else None
        self._sup, self._bsup = idx(self.suppress), idx(self.begin_suppress)
        self._not_lang = idx([t for t in range(self.V) if t not in set(self.lang_ids)]) if self.lang_ids else None
        self.B = 0

    def _alloc(self, B: int, T: int, steps: int):
        d, dev = self.d, self.dev

        def b16(*s):
            return torch.empty(*s, dtype=BF16, device=dev)
        self.B, self.T, self.steps = B, T, steps
        self.enc16 = b16(B * T, d)
        self.ckv = [b16(B * T, 2 * d) for _ in range(self.L)]
        self.cache = [b16(B, steps, 2 * d) for _ in range(self.L)]
        self.x32 = torch.empty(B, d, dtype=F32, device=dev)
        self.hb, self.q16, self.att = b16(B, d), b16(B, d), b16(B, d)
        self.ff = b16(B, self.ffn)
        self.lse = torch.empty(B, self.heads, 1, dtype=F32, device=dev)
        self.logits = torch.zeros(B, self.Vp, dtype=BF16, device=dev)
        self.nxt = torch.zeros(B, dtype=torch.int64, device=dev)

    def _step(self, tok: torch.Tensor, t: int) -> torch.Tensor:
        """Token ids `tok` [B] at decoder position t -> logits [B, Vp] for position t + 1."""
        B, d, T = self.B, self.d, self.T
        scale = 64 ** -0.5
        self.x32.copy_(self.emb32[tok] + self.pos32[t])                            # embedding lookup + learned position (index plumbing)
        for ly, cache, ckv in zip(self.layers, self.cache, self.ckv):
            H.layernorm_fwd(self.x32, ly["ln1"][0], ly["ln1"][1], 1e-5, y16=self.hb)
            H.gemm(self.hb, ly["wq"], self.q16, B, d, d, bias=ly["bq"])
            H.gemm(self.hb, ly["wkv"], cache[:, t], B, 2 * d, d, bias=ly["bkv"], ldc=self.steps * 2 * d)       # K | V of this position straight into the cache
            ad = H.attn_desc(self.q16, cache, cache, self.att, self.lse, batch=B, hq=self.heads, hkv=self.heads, sq=1, sk=t + 1, hd=64, scale=scale,
                             q_off=0, k_off=0, v_off=d, q_rs=d, k_rs=2 * d, v_rs=2 * d, o_rs=d, q_bs=d, k_bs=self.steps * 2 * d, v_bs=self.steps * 2 * d, o_bs=d)
            H.attention_fwd(ad)
            H.gemm(self.att, ly["wo"], self.x32, B, d, d, bias=ly["bo"], residual=self.x32)
            H.layernorm_fwd(self.x32, ly["ln2"][0], ly["ln2"][1], 1e-5, y16=self.hb)
            H.gemm(self.hb, ly["cwq"], self.q16, B, d, d, bias=ly["cbq"])
            ad = H.attn_desc(self.q16, ckv, ckv, self.att, self.lse, batch=B, hq=self.heads, hkv=self.heads, sq=1, sk=T, hd=64, scale=scale,
                             q_off=0, k_off=0, v_off=d, q_rs=d, k_rs=2 * d, v_rs=2 * d, o_rs=d, q_bs=d, k_bs=T * 2 * d, v_bs=T * 2 * d, o_bs=d)
            H.attention_fwd(ad)
            H.gemm(self.att, ly["cwo"], self.x32, B, d, d, bias=ly["cbo"], residual=self.x32)
            H.layernorm_fwd(self.x32, ly["ln3"][0], ly["ln3"][1], 1e-5, y16=self.hb)
            H.gemm(self.hb, ly["w1"], self.ff, B, self.ffn, d, bias=ly["b1"], act=1)
            H.gemm(self.ff, ly["w2"], self.x32, B, d, self.ffn, bias=ly["b2"], residual=self.x32)
        H.layernorm_fwd(self.x32, self.ln_f[0], self.ln_f[1], 1e-5, y16=self.hb)
        H.gemm(self.hb, self.emb16, self.logits, B, self.V, d, ldc=self.Vp)
        return self.logits

    @torch.no_grad()
    def generate(self, encoder: "WhisperEncoderHIP", mel: torch.Tensor, max_new_tokens: int = 128, collect_logits: bool = False,
                 forced_tokens: Optional[torch.Tensor] = None):
        """mel [B, n_mels, 3000] -> new token ids [B, n] (int64; init tokens stripped, rows padded with pad_token_id after their EOS);
        with collect_logits also the RAW logits of every generated position [n, B, V] and the init tokens [B, n_init].  `forced_tokens`
        [B, n] teacher-forces the continuation (parity tests compare per-step logits on the golden's own prefix)."""
        dev = self.dev
        B = mel.shape[0]
        with torch.cuda.device(dev):
            nt = len(encoder.cfg.target_layer_ids)
            taps = torch.empty(nt, B * encoder.T, encoder.d, dtype=BF16, device=dev)
            encoder.forward(mel.to(dev, F32).contiguous(), taps)
            n_init_max = 1 + (1 if self.lang_ids else 0) + (1 if self.no_ts_id is not None else 0)
            steps = min(self.Tmax, n_init_max + int(max_new_tokens))
            if (B, encoder.T, steps) != (self.B, getattr(self, "T", -1), getattr(self, "steps", -1)):
                self._alloc(B, encoder.T, steps)
            H.layernorm_fwd(encoder.last32, self.ln_post[0], self.ln_post[1], 1e-5, y16=self.enc16)
            for ly, ckv in zip(self.layers, self.ckv):
                H.gemm(self.enc16, ly["cwkv"], ckv, B * encoder.T, 2 * self.d, self.d, bias=ly["cbkv"])
            tok = torch.full((B,), self.start_id, dtype=torch.int64, device=dev)
            init = [tok.clone()]
            logits = self._step(tok, 0)
            t = 1
            if self.lang_ids:
                # language detection (generation_whisper.py `detect_language`): argmax over the language tokens at the position behind <start>
                H.mask_tokens_bf16(logits, self.Vp, B, self.V, self._not_lang)
                H.argmax_bf16(logits, self.Vp, B, self.V, self.nxt)
                tok = self.nxt.clone()
                init.append(tok.clone())
                logits = self._step(tok, t)
                t += 1
            if self.no_ts_id is not None:
                tok = torch.full((B,), int(self.no_ts_id), dtype=torch.int64, device=dev)
                init.append(tok.clone())
                logits = self._step(tok, t)
                t += 1
            n_new = min(int(max_new_tokens), self.Tmax - t, steps - t + 1)
            out = torch.full((B, max(n_new, 1)), self.pad_id, dtype=torch.int64, device=dev)
            finished = torch.zeros(B, dtype=torch.bool, device=dev)
            eos = torch.tensor(self.eos_ids, dtype=torch.int64, device=dev)
            raw = []
            made = 0
            for k in range(n_new):
                if collect_logits:
                    raw.append(logits[:, : self.V].clone())
                if self._sup is not None:
                    H.mask_tokens_bf16(logits, self.Vp, B, self.V, self._sup)
                if k == 0 and self._bsup is not None:
                    H.mask_tokens_bf16(logits, self.Vp, B, self.V, self._bsup)
                H.argmax_bf16(logits, self.Vp, B, self.V, self.nxt)
                pick = self.nxt if forced_tokens is None else forced_tokens[:, k].to(dev, torch.int64)
                nxt = torch.where(finished, torch.full_like(pick, self.pad_id), pick)
                out[:, k] = nxt
                made = k + 1
                finished |= (nxt.unsqueeze(1) == eos.unsqueeze(0)).any(dim=1)
                if k + 1 == n_new or ((k & 7) == 7 and bool(finished.all())):
                    break
                logits = self._step(nxt, t)
                t += 1
            out = out[:, :made]
            if bool(finished.all()) and made > 1:                                # trim the columns behind the last EOS
                last = int(((out.unsqueeze(2) == eos.view(1, 1, -1)).any(dim=2).int().argmax(dim=1) + 1).max())
                out = out[:, :last]
                raw = raw[:last]
        if collect_logits:
            return out, torch.stack(raw), torch.stack(init, dim=1)
        return out


# =========================================================================================== Q-Former connector
class QformerConnectorHIP:
    """Trainable connector (modeling_desta25.py:126-205, 587-606): the 4 taps are run as ONE batch of
    taps*B prompt sequences (same weights for every tap), hoisted after the encoder loop
    (mathematically identical), forward + hand-written backward.  The attention outputs are also kept UNROUNDED
    (fp32, `a_s32` / `a_c32`): the backward's delta = rowsum(dO * O) taken from the bf16-rounded O carries an error that is
    coherent over the 1500 keys of a cross-attention row and showed up as 10-13 % error on the deep layers' query-weight
    gradients (the reference's eager attention sums P * dP itself); with the fp32 O it is at the reference's own bf16 floor."""

    def __init__(self, cfg: DeSTA25Config, arena: ParamArena, device):
        self.cfg, self.arena, self.dev = cfg, arena, device
        # qformer_1: the whole connector.  orca_hybrid: the GLOBAL branch of ORCAHybridConnector (modeling_desta25.py:241-264, 318-334) is
        # the same Q-Former block under other tensor names with `orca_global_num_tokens` queries
        orca = cfg.connector_mode == "orca_hybrid"
        self.n_prompts = CON + ("global_queries." if orca else "layer_prompts.")
        self.n_weights = CON + ("global_layer_weights" if orca else "layer_weights")
        self.n_qf = CON + ("global_qformer.layer." if orca else "qformer.layer.")
        self.n_proj = CON + ("global_proj." if orca else "proj.")
        self.d, self.K, self.nt = cfg.encoder_config.d_model, (cfg.orca_global_num_tokens if orca else cfg.prompt_size), len(cfg.target_layer_ids)
        self.heads, self.T = cfg.encoder_config.encoder_attention_heads, cfg.encoder_config.max_source_positions
        self.inter, self.Lq, self.h = cfg.qformer_intermediate_size, cfg.qformer_num_hidden_layers, cfg.llm_config.hidden_size
        assert self.d // self.heads == 64 and self.d % 64 == 0 and self.inter % 64 == 0 and self.h % 64 == 0
        assert (self.K * self.d) % 64 == 0, "layer_prompts must tile the arena without padding"
        self.w16 = torch.empty(arena.numel, dtype=BF16, device=device)          # bf16 image of the arena (autocast copy)
        self.B = 0
        self.p_drop = 0.0                      # set per forward by the model (cfg.qformer_dropout in training mode)
        self.overlap_dw = True                 # weight gradients on a side stream beside the dX chain
        self.kv_side = True                    # every layer's K | V projection on a second stream beside the query path (A/B: bench.py --no-kv-side)
        self._kv_stream = None
        self.xattn_transposed = True           # cross-attention backward writes d(K|V) transposed + the bias sums itself (A/B: bench.py --attn-q64-two-kernels)
        self._dw_stream, self._dw_pending = None, False
        self.seed_base = 0
        # transposed bf16 weights for the dX GEMMs: name -> [in, out] (refreshed on the optimizer's side stream; reading W
        # itself as a transposed-storage operand measured 25-45 % slower per dX GEMM, tools/tn_bench.py)
        self.wT: Dict[str, torch.Tensor] = {}

    # -- views
    def P(self, name):
        return self.arena.param(name)

    def G(self, name):
        return self.arena.grad(name)

    def W16(self, name, rows=None):
        """bf16 copy of parameter `name`; rows != None widens the view over adjacent tensors (fused QKV)."""
        o = self.arena.offsets[name]
        shape = self.arena.shapes[name]
        r = shape[0] if rows is None else rows
        return self.w16[o:o + r * shape[1]].view(r, shape[1])

    def P32(self, name, n=None):
        o = self.arena.offsets[name]
        n = int(math.prod(self.arena.shapes[name])) if n is None else n
        return self.arena.params[o:o + n]

    def G32(self, name, n=None):
        o = self.arena.offsets[name]
        n = int(math.prod(self.arena.shapes[name])) if n is None else n
        return self.arena.grads[o:o + n]

    def refresh_weights(self):
        """Per step: bf16 image of all parameters + transposed copies for the dX GEMMs."""
        H.cast_bf16(self.arena.params, self.w16, self.arena.numel)
        d, inter = self.d, self.inter
        for i in range(self.Lq):
            p = f"{self.n_qf}{i}."
            for key, name, rows, cols in (
                    ("s.qkv", p + "attention.self.query.weight", 3 * d, d), ("s.o", p + "attention.output.dense.weight", d, d),
                    ("c.q", p + "crossattention.self.query.weight", d, d), ("c.o", p + "crossattention.output.dense.weight", d, d),
                    ("i", p + "intermediate.dense.weight", inter, d), ("o", p + "output.dense.weight", d, inter)):
                k = f"{i}.{key}"
                if k not in self.wT:
                    self.wT[k] = torch.empty(cols, rows, dtype=BF16, device=self.dev)
                H.transpose_to_bf16(self.W16(name, rows), rows, cols, self.wT[k], rows)
        if "proj" not in self.wT:
            self.wT["proj"] = torch.empty(d, self.h, dtype=BF16, device=self.dev)
        H.transpose_to_bf16(self.W16(self.n_proj + "1.weight"), self.h, d, self.wT["proj"], self.h)

    def _alloc(self, B: int):
        d, K, nt, T, dev, inter = self.d, self.K, self.nt, self.T, self.dev, self.inter
        self.B = B
        R, E = nt * B * K, nt * B * T
        self.R, self.E = R, E
        self.Rp, self.Ep, self.BKp = _r64(R), _r64(E), _r64(B * K)

        def b16(*s):
            return torch.empty(*s, dtype=BF16, device=dev)

        def f32(*s):
            return torch.empty(*s, dtype=F32, device=dev)
        self.x0_32, self.x0_16 = f32(R, d), b16(R, d)
        self.sv = []
        for _ in range(self.Lq):
            self.sv.append(dict(
                qkv=b16(R, 3 * d), a_s=b16(R, d), a_s32=f32(R, d), a_c32=f32(R, d), lse_s=f32(nt * B, self.heads, K), pre1=f32(R, d), st1=f32(R, 2), x1_32=f32(R, d), x1_16=b16(R, d),
                qc=b16(R, d), kv=b16(E, 2 * d), a_c=b16(R, d), lse_c=f32(nt * B, self.heads, K), pre2=f32(R, d), st2=f32(R, 2), x2_32=f32(R, d), x2_16=b16(R, d),
                hpre=b16(R, inter), hact=b16(R, inter), pre3=f32(R, d), st3=f32(R, 2), x3_32=f32(R, d), x3_16=b16(R, d)))
        self.mixed, self.st_p, self.pb = f32(B * K, d), f32(B * K, 2), b16(B * K, d)
        self.af = b16(B * K, self.h)
        # backward scratch
        self.g32a, self.g32b = f32(R, d), f32(R, d)
        self.dpre16, self.da, self.dq, self.dm16 = b16(R, d), b16(R, d), b16(R, d), b16(R, d)
        self.dqkv, self.dh = b16(R, 3 * d), b16(R, inter)
        self.dkv = b16(E, 2 * d)
        self.tA = b16(max(3 * d, inter, self.h) * max(self.Rp, self.BKp))     # transposed dY  [N, Rp]
        self.tB = b16(max(d, inter) * max(self.Rp, self.BKp))                  # transposed X   [K, Rp]
        self.tE = b16(d, self.Ep)                                              # enc^T, shared by all layers
        self.tKV = torch.zeros(2 * d, self.Ep, dtype=BF16, device=dev)         # d(K|V)^T; pad columns stay zero (the one-pass attention backward writes the E real ones only)
        self.dmixed = f32(B * K, d)
        self.dpb = b16(B * K, d)

    # -- forward
    def forward(self, enc_all: torch.Tensor, B: int) -> torch.Tensor:
        """enc_all [taps, B*T, d] bf16 -> audio features [B*K, h] bf16."""
        if B != self.B:
            self._alloc(B)
        d, K, nt, T, R, E = self.d, self.K, self.nt, self.T, self.R, self.E
        self.enc = enc_all.view(E, d)
        H.prompt_expand(self.P32(self.n_prompts + "0", nt * K * d), nt, B, K * d, self.x0_32, self.x0_16)
        x32, x16 = self.x0_32, self.x0_16
        scale = 64 ** -0.5
        pd = self.p_drop
        kv_ev = None
        if self.kv_side:
            # the K | V projections of the encoder states depend on nothing of the query path: all layers' projections go to a second
            # stream up front and run beside the chain of small (2048-row) kernels, which leave 40 % of the CUs idle
            if self._kv_stream is None:
                self._kv_stream = torch.cuda.Stream(device=self.dev)
            main = torch.cuda.current_stream(self.dev)
            self._kv_stream.wait_stream(main)
            kv_ev = []
            with torch.cuda.stream(self._kv_stream):
                for i in range(self.Lq):
                    p = f"{self.n_qf}{i}."
                    H.gemm(self.enc, self.W16(p + "crossattention.self.key.weight", 2 * d), self.sv[i]["kv"], E, 2 * d, d, bias=self.P32(p + "crossattention.self.key.bias", 2 * d))
                    ev = torch.cuda.Event()
                    ev.record(self._kv_stream)
                    kv_ev.append(ev)
        for i in range(self.Lq):
            p, s = f"{self.n_qf}{i}.", self.sv[i]
            sd = [site_seed(self.seed_base, 1, i, k) for k in range(5)]   # attn-self, out1, attn-cross, out2, out3
            s["seeds"], s["pd"] = sd, pd
            # self-attention over the K queries (bidirectional, H5)
            H.gemm(x16, self.W16(p + "attention.self.query.weight", 3 * d), s["qkv"], R, 3 * d, d, bias=self.P32(p + "attention.self.query.bias", 3 * d))
            ad = H.attn_desc(s["qkv"], s["qkv"], s["qkv"], s["a_s"], s["lse_s"], batch=nt * B, hq=self.heads, hkv=self.heads, sq=K, sk=K,
                             hd=64, scale=scale, q_off=0, k_off=d, v_off=2 * d, dropout_p=pd, dropout_seed=sd[0], o_f32=s["a_s32"])
            H.attention_fwd(ad)
            s["ad_s"] = ad
            H.gemm(s["a_s"], self.W16(p + "attention.output.dense.weight"), s["pre1"], R, d, d, bias=self.P32(p + "attention.output.dense.bias"), residual=x32,
                   dropout_p=pd, dropout_seed=sd[1])
            H.layernorm_fwd(s["pre1"], self.P32(p + "attention.output.LayerNorm.weight"), self.P32(p + "attention.output.LayerNorm.bias"), 1e-12,
                            y16=s["x1_16"], y32=s["x1_32"], stats=s["st1"])
            # cross-attention: K queries x T encoder states (unmasked)
            H.gemm(s["x1_16"], self.W16(p + "crossattention.self.query.weight"), s["qc"], R, d, d, bias=self.P32(p + "crossattention.self.query.bias"))
            if kv_ev is None:
                H.gemm(self.enc, self.W16(p + "crossattention.self.key.weight", 2 * d), s["kv"], E, 2 * d, d, bias=self.P32(p + "crossattention.self.key.bias", 2 * d))
            else:
                torch.cuda.current_stream(self.dev).wait_event(kv_ev[i])
            ad = H.attn_desc(s["qc"], s["kv"], s["kv"], s["a_c"], s["lse_c"], batch=nt * B, hq=self.heads, hkv=self.heads, sq=K, sk=T,
                             hd=64, scale=scale, q_off=0, k_off=0, v_off=d, dropout_p=pd, dropout_seed=sd[2], o_f32=s["a_c32"])
            H.attention_fwd(ad)
            s["ad_c"] = ad
            H.gemm(s["a_c"], self.W16(p + "crossattention.output.dense.weight"), s["pre2"], R, d, d, bias=self.P32(p + "crossattention.output.dense.bias"), residual=s["x1_32"],
                   dropout_p=pd, dropout_seed=sd[3])
            H.layernorm_fwd(s["pre2"], self.P32(p + "crossattention.output.LayerNorm.weight"), self.P32(p + "crossattention.output.LayerNorm.bias"), 1e-12,
                            y16=s["x2_16"], y32=s["x2_32"], stats=s["st2"])
            # FFN
            H.gemm(s["x2_16"], self.W16(p + "intermediate.dense.weight"), s["hact"], R, self.inter, d, bias=self.P32(p + "intermediate.dense.bias"), act=1, preact=s["hpre"])
            H.gemm(s["hact"], self.W16(p + "output.dense.weight"), s["pre3"], R, d, self.inter, bias=self.P32(p + "output.dense.bias"), residual=s["x2_32"],
                   dropout_p=pd, dropout_seed=sd[4])
            H.layernorm_fwd(s["pre3"], self.P32(p + "output.LayerNorm.weight"), self.P32(p + "output.LayerNorm.bias"), 1e-12,
                            y16=s["x3_16"], y32=s["x3_32"], stats=s["st3"])
            s["x_in32"], s["x_in16"] = x32, x16
            x32, x16 = s["x3_32"], s["x3_16"]
        self.qf_out = x32
        H.tap_mix_fwd(x32, self.P32(self.n_weights), nt, B, K, d, self.mixed)
        H.layernorm_fwd(self.mixed, self.P32(self.n_proj + "0.weight"), self.P32(self.n_proj + "0.bias"), 1e-5, y16=self.pb, stats=self.st_p)
        H.gemm(self.pb, self.W16(self.n_proj + "1.weight"), self.af, B * K, self.h, d, bias=self.P32(self.n_proj + "1.bias"))
        return self.af

    def __call__(self, encoder_hidden_states) -> torch.Tensor:
        """The reference's `QformerConnector.forward(encoder_hidden_states)` (modeling_desta25.py:178-205): a list with
        one [B, T, d] state per encoder layer (the target layers are picked here) -> [B, prompt_size, llm_hidden] bf16."""
        states = [encoder_hidden_states[i] for i in self.cfg.target_layer_ids]
        B, T, d = states[0].shape
        assert d == self.d, f"encoder width {d} != {self.d}"
        if T != self.T:                                   # the connector is agnostic to the number of encoder frames
            self.T, self.B = T, 0
        with torch.cuda.device(self.dev):
            enc_all = torch.stack([s.to(self.dev, BF16).reshape(B * T, d) for s in states]).contiguous()
            self.refresh_weights()
            return self.forward(enc_all, B).view(B, self.K, self.h)

    # -- backward helpers
    def _dW(self, dY, X, M, N, Kin, wname, bname, Mp, x_is_T=None):
        """grad(wname)[N,Kin] = dY[M,N]^T @ X[M,Kin];  grad(bname)[N] = colsum(dY).  bf16 operands."""
        gw = self.G(wname) if N == self.arena.shapes[wname][0] else self._gwide(wname, N)
        if M % 64 == 0 and x_is_T is None:
            # both operands in transposed storage ([M, N] and [M, Kin], reduction index slow): no transposes
            # (44 vs 59 us per dW at N=3840, Kin=1280, M=2048: tools/tn_bench.py).  Weight / bias gradients are leaves of
            # the backward graph: they run on a side stream next to the dX chain (small GEMMs that fill a fraction of
            # the chip each); `_join_dw` re-joins before any dY buffer is overwritten (every LayerNorm backward).
            side = self._dw_side()
            if side is not None:
                side.wait_stream(torch.cuda.current_stream(self.dev))
                with torch.cuda.stream(side):
                    H.gemm(dY, X, gw, N, Kin, M, trans_a=True, trans_b=True, lda=dY.shape[-1], ldb=X.shape[-1])
                    if bname is not None:
                        H.colsum(dY, M, N, dY.shape[-1], self.G32(bname, N), tag="ws_dw_side")
                self._dw_pending = True
                return
            H.gemm(dY, X, gw, N, Kin, M, trans_a=True, trans_b=True, lda=dY.shape[-1], ldb=X.shape[-1])
        else:
            tA = self.tA[: N * Mp].view(N, Mp)
            H.transpose_to_bf16(dY, M, N, tA, Mp, ld_in=dY.shape[-1])
            if x_is_T is None:
                tB = self.tB[: Kin * Mp].view(Kin, Mp)
                H.transpose_to_bf16(X, M, Kin, tB, Mp, ld_in=X.shape[-1])
            else:
                tB = x_is_T
            H.gemm(tA, tB, gw, N, Kin, Mp)
        if bname is not None:
            H.colsum(dY, M, N, dY.shape[-1], self.G32(bname, N))

    def _dw_side(self):
        if not self.overlap_dw:
            return None
        if self._dw_stream is None:
            self._dw_stream = torch.cuda.Stream(device=self.dev)
        return self._dw_stream

    def _join_dw(self):
        """Main stream waits for the weight-gradient kernels issued so far (before their dY inputs are overwritten)."""
        if self._dw_pending:
            torch.cuda.current_stream(self.dev).wait_stream(self._dw_stream)
            self._dw_pending = False

    def _drop_grad(self, dpre16, s, site):
        """Gradient w.r.t. a dense output that went through epilogue dropout: same mask, same 1/(1-p)."""
        if s["pd"] <= 0.0:
            return dpre16
        H.dropout_bf16(dpre16, self.dm16, self.R, self.d, self.d, s["pd"], s["seeds"][site])
        return self.dm16

    def _gwide(self, name, rows):
        o = self.arena.offsets[name]
        cols = self.arena.shapes[name][1]
        return self.arena.grads[o:o + rows * cols].view(rows, cols)

    def backward(self, d_af: torch.Tensor) -> None:
        """d_af [B*K, h] bf16 = dL/d audio_features  ->  gradients of every connector tensor (arena.grads)."""
        d, K, nt, T, R, E, B, inter, h = self.d, self.K, self.nt, self.T, self.R, self.E, self.B, self.inter, self.h
        BK = B * K
        # projector
        self._dW(d_af, self.pb, BK, h, d, self.n_proj + "1.weight", self.n_proj + "1.bias", self.BKp)
        H.gemm(d_af, self.wT["proj"], self.dpb, BK, d, h)
        H.layernorm_bwd(self.dpb, self.mixed, self.P32(self.n_proj + "0.weight"), self.st_p, dx32=self.dmixed,
                        dgamma=self.G32(self.n_proj + "0.weight"), dbeta=self.G32(self.n_proj + "0.bias"))
        dx = self.g32a                                                        # grad wrt current layer output (fp32 [R,d])
        H.tap_mix_bwd(self.qf_out, self.P32(self.n_weights), self.dmixed, nt, B, K, d, dx, self.G32(self.n_weights))
        other = self.g32b
        H.transpose_to_bf16(self.enc, E, d, self.tE, self.Ep)
        for i in reversed(range(self.Lq)):
            p, s = f"{self.n_qf}{i}.", self.sv[i]
            # --- FFN block: x3 = LN(pre3), pre3 = hact@Wo^T + b + x2
            dpre, dpre16, dh, da, dq, dqkv = other, self.dpre16, self.dh, self.da, self.dq, self.dqkv
            self._join_dw()
            H.layernorm_bwd(dx, s["pre3"], self.P32(p + "output.LayerNorm.weight"), s["st3"], dx32=dpre, dx16=dpre16,
                            dgamma=self.G32(p + "output.LayerNorm.weight"), dbeta=self.G32(p + "output.LayerNorm.bias"))
            dm = self._drop_grad(dpre16, s, 4)                                                   # grad of the dense output (through its dropout)
            self._dW(dm, s["hact"], R, d, inter, p + "output.dense.weight", p + "output.dense.bias", self.Rp)
            H.gemm(dm, self.wT[f"{i}.o"], dh, R, inter, d)
            H.gelu_bwd(s["hpre"], dh, dh, R * inter)
            self._dW(dh, s["x2_16"], R, inter, d, p + "intermediate.dense.weight", p + "intermediate.dense.bias", self.Rp)
            H.gemm(dh, self.wT[f"{i}.i"], dx, R, d, inter, residual=dpre)                      # dx := d x2_32
            # --- cross-attention block: x2 = LN(pre2), pre2 = a_c@Wo^T + b + x1
            self._join_dw()
            H.layernorm_bwd(dx, s["pre2"], self.P32(p + "crossattention.output.LayerNorm.weight"), s["st2"], dx32=dpre, dx16=dpre16,
                            dgamma=self.G32(p + "crossattention.output.LayerNorm.weight"), dbeta=self.G32(p + "crossattention.output.LayerNorm.bias"))
            dm = self._drop_grad(dpre16, s, 3)
            self._dW(dm, s["a_c"], R, d, d, p + "crossattention.output.dense.weight", p + "crossattention.output.dense.bias", self.Rp)
            H.gemm(dm, self.wT[f"{i}.c.o"], da, R, d, d)
            # key/value projections of the encoder states (no dX into the frozen Whisper states): their weight gradient wants
            # d(K|V) TRANSPOSED ([2d, E]) and their bias gradient its sums over the E rows
            xt = self.xattn_transposed and K <= 64 and T >= 256 and T % 4 == 0 and self.heads * 64 == d
            if xt:
                # the one-pass backward writes d(K|V) in that layout itself and sums the bias gradients on the way
                H.attention_bwd(s["ad_c"], da, dq, dkv_t=(self.tKV, self.Ep, self.G32(p + "crossattention.self.key.bias", 2 * d)))
            else:
                H.attention_bwd(s["ad_c"], da, dq, self.dkv, self.dkv, dk_off=0, dv_off=d)
            self._dW(dq, s["x1_16"], R, d, d, p + "crossattention.self.query.weight", p + "crossattention.self.query.bias", self.Rp)
            if not xt:
                H.transpose_to_bf16(self.dkv, E, 2 * d, self.tKV, self.Ep)
                H.colsum(self.dkv, E, 2 * d, 2 * d, self.G32(p + "crossattention.self.key.bias", 2 * d))
            # (this GEMM on the dW side stream beside the dX chain: connector backward 6.11 -> 6.29 ms, slower; on a third stream with a
            #  double-buffered d(K|V)^T: 6.01 / 6.11 vs 6.09 / 6.07 ms, equal — the backward is bound by its total work, not by exposed latency)
            H.gemm(self.tKV, self.tE, self._gwide(p + "crossattention.self.key.weight", 2 * d), 2 * d, d, self.Ep)
            H.gemm(dq, self.wT[f"{i}.c.q"], dx, R, d, d, residual=dpre)                         # dx := d x1_32
            # --- self-attention block: x1 = LN(pre1), pre1 = a_s@Wo^T + b + x_in
            self._join_dw()
            H.layernorm_bwd(dx, s["pre1"], self.P32(p + "attention.output.LayerNorm.weight"), s["st1"], dx32=dpre, dx16=dpre16,
                            dgamma=self.G32(p + "attention.output.LayerNorm.weight"), dbeta=self.G32(p + "attention.output.LayerNorm.bias"))
            dm = self._drop_grad(dpre16, s, 1)
            self._dW(dm, s["a_s"], R, d, d, p + "attention.output.dense.weight", p + "attention.output.dense.bias", self.Rp)
            H.gemm(dm, self.wT[f"{i}.s.o"], da, R, d, d)
            H.attention_bwd(s["ad_s"], da, dqkv, dqkv, dqkv, dq_off=0, dk_off=d, dv_off=2 * d)
            self._dW(dqkv, s["x_in16"], R, 3 * d, d, p + "attention.self.query.weight", p + "attention.self.query.bias", self.Rp)
            H.gemm(dqkv, self.wT[f"{i}.s.qkv"], dx, R, d, 3 * d, residual=dpre)                # dx := d x_in32
        H.prompt_grad(dx, nt, B, K * d, self.G32(self.n_prompts + "0", nt * K * d))
        self._join_dw()


# =========================================================================================== ORCA hybrid
class OrcaHIP:
    """ORCA hybrid: forward of the local branch of `ORCAHybridConnector` (modeling_desta25.py:336-352),
    of `ORCAGatedCrossAttention` behind every decoder layer (:395-490, installed by `_enable_orca_deep_injection` :1052-1143) and of
    `compute_orca_losses` (:1159-1206), composed from the C-ABI entry points of the qformer_1 path (GEMM, flash attention, LayerNorm)
    plus the row-wise `desta_orca_*` kernels.  The global branch is `QformerConnectorHIP` under the ORCA tensor names.
    BACKWARD (round 4, second slice): hand-written like the rest of the path — `inject_bwd` (gate, gate MLP, LayerNorm, out-proj,
    attention, q / k|v projections, alignment loss; called by the decoder's backward behind every layer), `backward_tail` (rotation
    transpose, the two similarity losses, local branch: LayerNorm, Conv1d as im2col dW + col2im dX, Linear, tap mix; then the global
    branch = `QformerConnectorHIP.backward`).  Pinned to the reference's own classes and autograd at tiny size
    (tests/golden/ref_orca_tiny.safetensors, tests/test_gpu_orca.py).  LayerNorm backward is built for hidden <= 2048."""

    def __init__(self, cfg: DeSTA25Config, connector: "QformerConnectorHIP", device):
        c = cfg.llm_config
        self.cfg, self.con, self.dev = cfg, connector, device
        self.h, self.d, self.nt = c.hidden_size, cfg.encoder_config.d_model, len(cfg.target_layer_ids)
        self.heads, self.L = c.num_attention_heads, c.num_hidden_layers
        self.hd = self.h // self.heads
        if self.hd > 128 or self.hd * self.heads != self.h:
            raise NotImplementedError(f"orca_hybrid: cross-attention head size {self.hd} (hidden {self.h} / {self.heads} heads); up to 128 is built")
        # nn.MultiheadAttention(embed_dim = hidden, num_heads = the LLM's): head size hidden / heads, e.g. 2560 / 32 = 80 for Qwen3-4B.  The
        # flash kernels are built for 64 and 128: other sizes run zero-padded to the next of the two (`hdp`): padded q / k columns add
        # nothing to a score, padded v columns give zero outputs that meet zero out-proj columns; the softmax scale stays hd ** -0.5.
        # The padded bf16 operands are rebuilt with the other bf16 copies (`refresh_weights`), weight gradients are un-padded into the arena.
        self.hdp = 64 if self.hd <= 64 else 128
        self.hp, self.padded = self.heads * self.hdp, self.hdp != self.hd
        self.wp: List[dict] = []
        self.k, self.stride = cfg.orca_local_kernel_size, cfg.orca_local_downsample
        self.pad = self.k // 2
        assert self.h % 64 == 0 and (self.h // 4) % 4 == 0
        # the reference reads `llm_config.rope_theta` (modeling_desta25.py:1087; 4.x config attribute); transformers 5.x keeps it under
        # rope_parameters and the reference's getattr then falls back to 10000.0 — LLMConfig carries the model's value (4.x semantics)
        self.rope_theta = float(cfg.extra.get("orca_rope_theta", c.rope_theta))
        self.conv_w = None
        self.B = 0
        self._tb: Dict[tuple, torch.Tensor] = {}
        self._lidx: Dict[int, torch.Tensor] = {}

    def local_index(self, Tl: int) -> Optional[torch.Tensor]:
        """Rows of the local tokens the global / local orthogonality loss reads: all of them up to 100, else the reference's uniform
        sample of 100 (:1190-1194), built like the reference's (`torch.linspace(..., dtype=torch.long, device=l_norm.device)`) on the
        device, once per Tl, int32.  Shared by `losses` and `backward_tail`."""
        if Tl <= 100:
            return None
        if Tl not in self._lidx:
            self._lidx[Tl] = torch.linspace(0, Tl - 1, 100, dtype=torch.long, device=self.dev).to(torch.int32)
        return self._lidx[Tl]

    def refresh_weights(self) -> None:
        """bf16 operand of the Conv1d as an im2col GEMM: [out, in, k] -> [out, k * in] (tap-major rows of the padded token stream)."""
        if self.cfg.orca_local_enabled:
            w = self.con.arena.param(CON + "local_conv.weight")
            self.conv_w = w.permute(0, 2, 1).reshape(self.h, self.k * self.h).to(BF16).contiguous()
        if self.padded and self.cfg.orca_deep_injection_enabled:
            con, h, hp, nh, hd, hdp, dev = self.con, self.h, self.hp, self.heads, self.hd, self.hdp, self.dev
            if not self.wp:
                self.wp = [dict(wq=torch.zeros(hp, h, dtype=BF16, device=dev), wkv=torch.zeros(2 * hp, h, dtype=BF16, device=dev),
                                wo=torch.zeros(h, hp, dtype=BF16, device=dev), bq=torch.zeros(hp, dtype=F32, device=dev),
                                bkv=torch.zeros(2 * hp, dtype=F32, device=dev)) for _ in range(self.L)]
            for l, t in enumerate(self.wp):
                q = f"orca_cross_attns.{l}."
                w_in, b_in = con.W16(q + "cross_attn.in_proj_weight"), con.P32(q + "cross_attn.in_proj_bias")
                t["wq"].view(nh, hdp, h)[:, :hd].copy_(w_in[:h].view(nh, hd, h))
                t["wkv"].view(2 * nh, hdp, h)[:, :hd].copy_(w_in[h:].view(2 * nh, hd, h))
                t["bq"].view(nh, hdp)[:, :hd].copy_(b_in[:h].view(nh, hd))
                t["bkv"].view(2 * nh, hdp)[:, :hd].copy_(b_in[h:].view(2 * nh, hd))
                t["wo"].view(h, nh, hdp)[:, :, :hd].copy_(con.W16(q + "cross_attn.out_proj.weight").view(h, nh, hd))

    def _attn_weights(self, l: int):
        """(W_q [hp, h], W_k|v [2 hp, h], b_q, b_k|v, W_o [h, hp]) of layer l's cross-attention in the width the attention kernel runs at."""
        if self.padded:
            t = self.wp[l]
            return t["wq"], t["wkv"], t["bq"], t["bkv"], t["wo"]
        con, h, q = self.con, self.h, f"orca_cross_attns.{l}."
        w_in, b_in = con.W16(q + "cross_attn.in_proj_weight"), con.P32(q + "cross_attn.in_proj_bias")
        return w_in[:h], w_in[h:], b_in[:h], b_in[h:], con.W16(q + "cross_attn.out_proj.weight")

    def _alloc(self, B: int, T: int) -> None:
        dev, h = self.dev, self.h
        self.B, self.T = B, T
        self.Tl = (T + 2 * self.pad - self.k) // self.stride + 1
        self.fused = torch.empty(B * T, self.d, dtype=BF16, device=dev)
        self.loc_in = torch.zeros(B, T + 2 * self.pad, h, dtype=BF16, device=dev)      # zero rows = the convolution's padding
        self.conv_out = torch.empty(B * self.Tl, h, dtype=F32, device=dev)
        self.local16 = torch.empty(B * self.Tl, h, dtype=BF16, device=dev)

    # -- views of the ORCA tensors in the connector's arena
    def G32(self, name, n=None):
        return self.con.G32(name, n)

    def Gw(self, name):
        return self.con.arena.grad(name)

    def _tbuf(self, tag: str, rows: int, Mp: int) -> torch.Tensor:
        """Zero-initialised [rows, Mp] bf16 scratch for a transposed operand (columns past the token count stay zero: only [0, M) is written)."""
        key = (tag, rows, Mp)
        if key not in self._tb:
            self._tb[key] = torch.zeros(rows, Mp, dtype=BF16, device=self.dev)
        return self._tb[key]

    def _transposed(self, tag: str, X: torch.Tensor, M: int, cols: int) -> torch.Tensor:
        t = self._tbuf(tag, cols, _r64(M))
        H.transpose_to_bf16(X, M, cols, t, t.shape[1], ld_in=X.shape[-1])
        return t

    def _dW(self, dY: torch.Tensor, X: torch.Tensor, M: int, N: int, Kin: int, gw: torch.Tensor, gb: Optional[torch.Tensor],
            xT: Optional[torch.Tensor] = None) -> None:
        """gw [N, Kin] (fp32, written) = dY[M, N]^T X[M, Kin];  gb [N] = column sums of dY.  Large products (the 4096-wide projections of a
        full-size decoder): explicit bf16 transposes + the 256x256 NT kernel (217 -> 167 us at 4096 x 4096 x 5120, 152 with X^T shared:
        tools/orca_dw_bench.py; `xT` = an X^T [Kin, r64(M)] the caller already holds).  Small ones: both operands in transposed storage
        (the token index is the reduction index) on the 128x128 kernel, a token count that is not a multiple of 64 through zero-padded copies."""
        if N * Kin >= (1 << 23) and M >= 1024:
            tA = self._transposed("dY", dY, M, N)
            tB = xT if xT is not None else self._transposed("X", X, M, Kin)
            H.gemm(tA, tB, gw, N, Kin, tA.shape[1])
        elif M % 64 != 0:
            Mp = _r64(M)
            dYp = torch.zeros(Mp, N, dtype=BF16, device=self.dev)
            Xp = torch.zeros(Mp, Kin, dtype=BF16, device=self.dev)
            dYp[:M].copy_(dY[:M])
            Xp[:M].copy_(X[:M])
            H.gemm(dYp, Xp, gw, N, Kin, Mp, trans_a=True, trans_b=True, lda=N, ldb=Kin)
        else:
            H.gemm(dY, X, gw, N, Kin, M, trans_a=True, trans_b=True, lda=N, ldb=Kin)
        if gb is not None:
            H.colsum(dY, M, N, N, gb)

    def local_forward(self, enc_all: torch.Tensor, B: int) -> torch.Tensor:
        """enc_all [taps, B*T, d] bf16 -> local tokens [B*T', h] bf16."""
        con, h, d = self.con, self.h, self.d
        T = enc_all.shape[1] // B
        if not self.cfg.orca_local_enabled:                                     # ablation (:336, :352): global tokens only
            self.B, self.T, self.Tl = B, T, 0
            return None
        if (B, T) != (self.B, getattr(self, "T", -1)):
            self._alloc(B, T)
        if self.conv_w is None:
            self.refresh_weights()
        H.orca_local_mix(enc_all, con.P32(CON + "local_layer_weights"), self.nt, B * T, d, self.fused)
        Tp = T + 2 * self.pad
        H.gemm(self.fused, con.W16(CON + "local_proj_in.weight"), self.loc_in[:, self.pad:], T, h, d, bias=con.P32(CON + "local_proj_in.bias"),
               batch=B, stride_a=T * d, stride_c=Tp * h, ldc=h)
        # Conv1d(k, stride, pad) over time as a zero-copy im2col GEMM: output t' reads rows [t' stride, t' stride + k) of the padded stream
        H.gemm(self.loc_in, self.conv_w, self.conv_out, self.Tl, h, self.k * h, lda=self.stride * h, ldc=h, bias=con.P32(CON + "local_conv.bias"),
               batch=B, stride_a=Tp * h, stride_c=self.Tl * h)
        self.local_st = torch.empty(B * self.Tl, 2, dtype=F32, device=self.dev)
        H.layernorm_fwd(self.conv_out, con.P32(CON + "local_ln.weight"), con.P32(CON + "local_ln.bias"), 1e-5, y16=self.local16, stats=self.local_st)
        self.enc_all = enc_all
        return self.local16

    # -- deep injection
    def begin(self, global16: torch.Tensor, local16: Optional[torch.Tensor], B: int, S: int, spans, training: bool, save: bool = False,
              keep_kv: bool = False) -> None:
        """Audio tokens the gated cross-attention of every layer attends to (modeling_desta25.py:792-806): the local tokens, or
        global | local with `orca_global_cross_attn`; rotated ONCE (the rotation does not depend on the layer, :422-438)."""
        cfg, h, dev = self.cfg, self.h, self.dev
        self.audio = None
        self.aligns: List[torch.Tensor] = []
        self.save, self.sv = bool(save), [dict() for _ in range(self.L)]
        self.kv_layers: Optional[List[Optional[torch.Tensor]]] = [None] * self.L if keep_kv else None
        self.decoding = False
        self.global16, self.local16_in = global16, local16
        if not cfg.orca_deep_injection_enabled:
            return
        Kg = cfg.orca_global_num_tokens
        if cfg.orca_global_cross_attn:
            g3 = global16.view(B, Kg, h)
            a = torch.cat([g3, local16.view(B, -1, h)], dim=1).contiguous() if local16 is not None else g3.contiguous()
        else:
            a = local16.view(B, -1, h) if local16 is not None else None
        if a is None or a.shape[1] == 0:
            return
        Ta = a.shape[1]
        self.Ta, self.M, self.Bq, self.S = Ta, B * S, B, S
        self.audio = torch.empty(B * Ta, h, dtype=BF16, device=dev)
        H.orca_rope(a, self.audio, B, Ta, h, self.rope_theta, cfg.orca_audio_position_scale, round_cos_sin=True)
        M = B * S
        hp = self.hp
        if self.padded and not self.wp:
            self.refresh_weights()
        self.q16, self.att16 = torch.empty(M, hp, dtype=BF16, device=dev), torch.empty(M, hp, dtype=BF16, device=dev)
        self.kv16 = torch.empty(B * Ta, 2 * hp, dtype=BF16, device=dev)
        self.lse = torch.empty(B, self.heads, S, dtype=F32, device=dev)
        self.cross32, self.cross16 = torch.empty(M, h, dtype=F32, device=dev), torch.empty(M, h, dtype=BF16, device=dev)
        self.g1 = torch.empty(M, h // 4, dtype=BF16, device=dev)
        self.spans = None
        if training:
            # per-layer alignment loss (:459-488): transcription spans when the batch carries any, else the whole sequence
            if spans is not None and len(spans) > 0:
                ok = [(r, s0, s1) for r, s0, s1 in spans if s0 < s1 and s1 <= S]
                self.spans = torch.tensor(ok, dtype=torch.int32, device=dev).reshape(-1, 3) if ok else False
            else:
                self.spans = torch.tensor([(b, 0, S) for b in range(B)], dtype=torch.int32, device=dev)

    def _row_buffers(self, S: int) -> None:
        """The per-row buffers of `inject` for S rows per sequence."""
        B, h, dev = self.Bq, self.h, self.dev
        M = B * S
        self.M, self.S = M, S
        self.q16, self.att16 = torch.empty(M, self.hp, dtype=BF16, device=dev), torch.empty(M, self.hp, dtype=BF16, device=dev)
        self.lse = torch.empty(B, self.heads, S, dtype=F32, device=dev)
        self.cross32, self.cross16 = torch.empty(M, h, dtype=F32, device=dev), torch.empty(M, h, dtype=BF16, device=dev)
        self.g1 = torch.empty(M, h // 4, dtype=BF16, device=dev)

    def begin_chunk(self, ci: int, Cc: int) -> None:
        """generate() with a chunked prompt pass (`begin(..., S = the first chunk's positions, keep_kv=True)`): chunk ci injects into
        Cc rows per sequence.  The first chunk projects every layer's audio K|V into `kv_layers`; later chunks reuse it, as the
        decode steps do.  `begin_decode` still follows the last chunk."""
        if self.audio is None:
            return
        self.decoding = ci > 0                                               # (`inject`: take K|V from `kv_layers`)
        if Cc != self.S:
            self.q16 = self.att16 = self.lse = self.cross32 = self.cross16 = self.g1 = None     # free before the new ones are made
            self._row_buffers(Cc)

    def begin_decode(self) -> None:
        """generate(): after the prompt pass (`begin(..., keep_kv=True)` + `inject` per layer) every decode step injects into ONE new
        row per sequence; the audio keys / values of each layer do not change between steps and stay in `kv_layers`."""
        if self.audio is None:
            return
        self.decoding = True
        self._row_buffers(1)

    def inject(self, l: int, x: torch.Tensor) -> None:
        """x [B*S, h] bf16 = output of decoder layer l (batch-major rows), updated IN PLACE: x + sigmoid(gate(x)) * LN(cross_attn(x, audio))."""
        if self.audio is None:
            return
        con, h, M, B, S, Ta, dev = self.con, self.h, self.M, self.Bq, self.S, self.Ta, self.dev
        p = f"orca_cross_attns.{l}."
        hp = self.hp
        w_q, w_kv, b_q, b_kv, w_o = self._attn_weights(l)
        if self.spans is not None and self.spans is not False:
            n = min(B, self.spans.shape[0])                                      # "audio_pooled may have different batch size, align by taking first N"
            out = torch.empty(n, dtype=F32, device=dev)
            H.orca_align(self.audio, Ta, x, h, S * h, h, self.spans, n, out)
            self.aligns.append(out)
        if self.save:
            # a training forward keeps what the hand-written backward of this layer's injection needs (bf16 unless noted): the layer
            # output BEFORE the injection, q, k|v, the attention output + lse, the out-proj output (fp32) with its LayerNorm statistics,
            # its normalised form, the gate MLP's pre-activation / activation, the gate (fp32)
            s = self.sv[l]
            s["xpre"] = x.clone()
            q16, kv16, att16 = torch.empty(M, hp, dtype=BF16, device=dev), torch.empty(B * Ta, 2 * hp, dtype=BF16, device=dev), torch.empty(M, hp, dtype=BF16, device=dev)
            lse, cross32, cross16 = torch.empty(B, self.heads, S, dtype=F32, device=dev), torch.empty(M, h, dtype=F32, device=dev), torch.empty(M, h, dtype=BF16, device=dev)
            g1, g1pre = torch.empty(M, h // 4, dtype=BF16, device=dev), torch.empty(M, h // 4, dtype=BF16, device=dev)
            st, gate = torch.empty(M, 2, dtype=F32, device=dev), torch.empty(M, dtype=F32, device=dev)
            s.update(q16=q16, kv16=kv16, att16=att16, lse=lse, cross32=cross32, cross16=cross16, g1=g1, g1pre=g1pre, st=st, gate=gate)
        else:
            q16, kv16, att16, lse, cross32, cross16, g1, g1pre, st, gate = (self.q16, self.kv16, self.att16, self.lse, self.cross32, self.cross16, self.g1,
                                                                            None, None, None)
        H.gemm(x, w_q, q16, M, hp, h, bias=b_q)
        if self.decoding:
            kv16 = self.kv_layers[l]                                             # projected in the prompt pass
        else:
            if self.kv_layers is not None:
                kv16 = self.kv_layers[l] = torch.empty(B * Ta, 2 * hp, dtype=BF16, device=dev)
            H.gemm(self.audio, w_kv, kv16, B * Ta, 2 * hp, h, bias=b_kv)
        ad = H.attn_desc(q16, kv16, kv16, att16, lse, batch=B, hq=self.heads, hkv=self.heads, sq=S, sk=Ta, hd=self.hdp,
                         scale=self.hd ** -0.5, q_off=0, k_off=0, v_off=hp)
        H.attention_fwd(ad)
        H.gemm(att16, w_o, cross32, M, h, hp, bias=con.P32(p + "cross_attn.out_proj.bias"))
        H.layernorm_fwd(cross32, con.P32(p + "ln.weight"), con.P32(p + "ln.bias"), 1e-5, y16=cross16, stats=st)
        H.gemm(x, con.W16(p + "gate_proj.0.weight"), g1, M, h // 4, h, bias=con.P32(p + "gate_proj.0.bias"), act=1, preact=g1pre)
        H.orca_gate_residual(x, h, cross16, g1, con.P32(p + "gate_proj.2.weight"), con.P32(p + "gate_proj.2.bias"), M, h, h // 4, gate_out=gate)
        if self.save:
            self.sv[l]["ad"] = ad

    # -- backward
    def begin_backward(self) -> None:
        h, dev = self.h, self.dev
        Kg = self.cfg.orca_global_num_tokens
        self.dglobal32 = torch.zeros(self.B * Kg, h, dtype=F32, device=dev)
        self.dlocal32 = torch.zeros(self.B * self.Tl, h, dtype=F32, device=dev) if self.Tl > 0 else None
        self.audioT = None
        if self.audio is not None:
            self.d_audio32 = torch.zeros(self.Bq * self.Ta, h, dtype=F32, device=dev)
            if 2 * self.hp * h >= (1 << 23) and self.Bq * self.Ta >= 1024:        # X^T of every layer's k|v weight gradient (`_dW`)
                self.audioT = self._transposed("audio", self.audio, self.Bq * self.Ta, h)

    def inject_bwd(self, l: int, dx: torch.Tensor) -> None:
        """dx [B*S, h] bf16 = d(loss) / d(output of decoder layer l AFTER its injection), updated IN PLACE to the gradient w.r.t. the output
        BEFORE it; the injection's parameter gradients go to the arena, the gradient of the rotated audio tokens accumulates in fp32."""
        if self.audio is None:
            return
        con, h, M, B, S, Ta, dev, s = self.con, self.h, self.M, self.Bq, self.S, self.Ta, self.dev, self.sv[l]
        p = f"orca_cross_attns.{l}."
        hp, nh, hd, hdp = self.hp, self.heads, self.hd, self.hdp
        w_q, w_kv, _, _, w_o = self._attn_weights(l)
        gw_in, gb_in = self.Gw(p + "cross_attn.in_proj_weight"), self.G32(p + "cross_attn.in_proj_bias")
        gw_o = self.Gw(p + "cross_attn.out_proj.weight")
        if self.padded:                                                       # weight gradients at the padded width, un-padded into the arena below
            gq_p, gkv_p = torch.empty(hp, h, dtype=F32, device=dev), torch.empty(2 * hp, h, dtype=F32, device=dev)
            gbq_p, gbkv_p, go_p = torch.empty(hp, dtype=F32, device=dev), torch.empty(2 * hp, dtype=F32, device=dev), torch.empty(h, hp, dtype=F32, device=dev)
        else:
            gq_p, gkv_p, gbq_p, gbkv_p, go_p = gw_in[:h], gw_in[h:], gb_in[:h], gb_in[h:], gw_o

        def b16(*sh):
            return torch.empty(*sh, dtype=BF16, device=dev)
        dc16, dg2 = b16(M, h), torch.empty(M, dtype=F32, device=dev)
        H.orca_gate_residual_bwd(dx, h, s["cross16"], s["gate"], M, h, dc16, dg2)
        # gate MLP: Linear(h, h/4) -> GELU -> Linear(h/4, 1)
        dpre16 = b16(M, h // 4)
        H.orca_gate_mlp_bwd(dg2, s["g1pre"], s["g1"], con.P32(p + "gate_proj.2.weight"), M, h // 4, dpre16,
                            self.G32(p + "gate_proj.2.weight"), self.G32(p + "gate_proj.2.bias"))
        self._dW(dpre16, s["xpre"], M, h // 4, h, self.Gw(p + "gate_proj.0.weight"), self.G32(p + "gate_proj.0.bias"))
        # LayerNorm(cross) -> out_proj -> attention -> q / k|v projections
        dcross16 = b16(M, h)
        H.layernorm_bwd(dc16, s["cross32"], con.P32(p + "ln.weight"), s["st"], dx16=dcross16, dgamma=self.G32(p + "ln.weight"), dbeta=self.G32(p + "ln.bias"))
        self._dW(dcross16, s["att16"], M, h, hp, go_p, self.G32(p + "cross_attn.out_proj.bias"))
        datt16, dq16, dkv16 = b16(M, hp), b16(M, hp), b16(B * Ta, 2 * hp)
        H.gemm(dcross16, w_o, datt16, M, hp, h, trans_b=True, ldb=hp)
        H.attention_bwd(s["ad"], datt16, dq16, dkv16, dkv16, dk_off=0, dv_off=hp)
        self._dW(dq16, s["xpre"], M, hp, h, gq_p, gbq_p)
        self._dW(dkv16, self.audio, B * Ta, 2 * hp, h, gkv_p, gbkv_p, xT=self.audioT)
        if self.padded:
            gw_in[:h].view(nh, hd, h).copy_(gq_p.view(nh, hdp, h)[:, :hd])
            gw_in[h:].view(2 * nh, hd, h).copy_(gkv_p.view(2 * nh, hdp, h)[:, :hd])
            gb_in[:h].view(nh, hd).copy_(gbq_p.view(nh, hdp)[:, :hd])
            gb_in[h:].view(2 * nh, hd).copy_(gbkv_p.view(2 * nh, hdp)[:, :hd])
            gw_o.view(h, nh, hd).copy_(go_p.view(h, nh, hdp)[:, :, :hd])
        H.gemm(dkv16, w_kv, self.d_audio32, B * Ta, h, 2 * hp, trans_b=True, ldb=h, residual=self.d_audio32)
        # into the layer output's gradient: the alignment loss of this layer (on the hidden states the injection READ), q path, gate path
        if self.spans is not None and self.spans is not False and self.aligns:
            n = min(B, self.spans.shape[0])
            coef = self.cfg.orca_align_weight_local / (len(self.aligns) * n)
            H.orca_align_bwd(self.audio, Ta, s["xpre"], h, S * h, h, self.spans, n, coef, dx, h, S * h)
        H.gemm(dq16, w_q, dx, M, h, hp, trans_b=True, ldb=h, residual=dx)
        H.gemm(dpre16, con.W16(p + "gate_proj.0.weight"), dx, M, h, h // 4, trans_b=True, ldb=h, residual=dx)
        self.sv[l] = {}                                                        # activations of this layer are dead

    def backward_tail(self, d_af: torch.Tensor) -> None:
        """d_af [B*Kg, h] bf16 = gradient of the spliced global tokens (from the decoder's input gradient).  Adds the deep injection's
        audio gradient (rotated back), the diversity / orthogonality losses, then runs the local branch's and the global branch's
        backward: every ORCA / connector gradient of the arena is written."""
        cfg, con, h, d, dev, B = self.cfg, self.con, self.h, self.d, self.dev, self.B
        Kg, Tl, T = cfg.orca_global_num_tokens, self.Tl, self.T
        g16, loc16 = self.global16, self.local16_in
        if self.audio is not None:
            H.orca_rope_bwd(self.d_audio32, B, self.Ta, h, self.rope_theta, cfg.orca_audio_position_scale, True,
                            Kg if cfg.orca_global_cross_attn else 0, self.dglobal32, self.dlocal32)
        H.orca_sim_loss_bwd(g16, None, Kg, g16, None, Kg, B, Kg, Kg, h, True, cfg.orca_ortho_diversity_weight / (B * Kg * Kg), self.dglobal32)
        if loc16 is None:                                                        # orca_local_enabled = False: only the global branch is left
            con.backward((self.dglobal32 + d_af.float()).to(BF16))
            return
        idx = self.local_index(Tl)
        ny = Tl if idx is None else idx.numel()
        assert ny <= 128
        co = cfg.orca_ortho_weight_qformer_local / (B * Kg * ny)
        H.orca_sim_loss_bwd(g16, None, Kg, loc16, idx, Tl, B, Kg, ny, h, False, co, self.dglobal32)
        H.orca_sim_loss_bwd(loc16, idx, Tl, g16, None, Kg, B, ny, Kg, h, False, co, self.dlocal32)
        # ---- local branch: LayerNorm -> Conv1d -> Linear -> tap mix
        k, st_, pad = self.k, self.stride, self.pad
        Tp = T + 2 * pad
        dconv16 = torch.empty(B * Tl, h, dtype=BF16, device=dev)
        H.layernorm_bwd(self.dlocal32, self.conv_out, con.P32(CON + "local_ln.weight"), self.local_st, dx16=dconv16,
                        dgamma=self.G32(CON + "local_ln.weight"), dbeta=self.G32(CON + "local_ln.bias"))
        # dW of the convolution = dY^T im2col(x): the im2col rows are MATERIALISED here (a strided copy, no arithmetic): the token
        # reduction wants rows in multiples of 64 and one contiguous operand over the batch
        xcol = self.loc_in.as_strided((B, Tl, k * h), (Tp * h, st_ * h, 1)).reshape(B * Tl, k * h).contiguous()
        gwc = torch.empty(h, k * h, dtype=F32, device=dev)
        self._dW(dconv16, xcol, B * Tl, h, k * h, gwc, self.G32(CON + "local_conv.bias"))
        self.Gw(CON + "local_conv.weight").copy_(gwc.view(h, k, h).permute(0, 2, 1))          # [out, k, in] -> the parameter's [out, in, k]
        dcol16 = torch.empty(B * Tl, k * h, dtype=BF16, device=dev)
        H.gemm(dconv16, self.conv_w, dcol16, B * Tl, k * h, h, trans_b=True, ldb=k * h)
        dpad16 = torch.empty(B, Tp, h, dtype=BF16, device=dev)
        H.orca_col2im_add(dcol16, B, Tl, Tp, h, k, st_, dpad16)
        dloc_in = dpad16[:, pad:pad + T].reshape(B * T, h).contiguous()
        self._dW(dloc_in, self.fused, B * T, h, d, self.Gw(CON + "local_proj_in.weight"), self.G32(CON + "local_proj_in.bias"))
        dfused16 = torch.empty(B * T, d, dtype=BF16, device=dev)
        H.gemm(dloc_in, con.W16(CON + "local_proj_in.weight"), dfused16, B * T, d, h, trans_b=True, ldb=d)
        H.orca_local_mix_bwd(dfused16, self.enc_all, con.P32(CON + "local_layer_weights"), self.nt, B * T, d, self.G32(CON + "local_layer_weights"))
        # ---- global branch (the Q-Former under the ORCA names): spliced-token gradient + what the losses / the injection added
        dg = (self.dglobal32 + d_af.float()).to(BF16)
        con.backward(dg)

    def losses(self, global16: torch.Tensor, local16: Optional[torch.Tensor], B: int) -> "OrderedDict[str, torch.Tensor]":
        """`compute_orca_losses` (:1159-1206): 0-d fp32 device tensors, weighted like the reference's."""
        cfg, h, dev = self.cfg, self.h, self.dev
        Kg = cfg.orca_global_num_tokens
        out: "OrderedDict[str, torch.Tensor]" = OrderedDict()
        part = torch.empty(B * Kg, dtype=F32, device=dev)
        H.orca_sim_loss(global16, global16, None, B, Kg, Kg, Kg, h, True, part)
        out["L_ortho_diversity"] = cfg.orca_ortho_diversity_weight * part.sum() / (B * Kg * Kg)
        if local16 is not None:
            Tl = local16.shape[0] // B
            idx = self.local_index(Tl)                                            # uniform sample of 100 local tokens above 100 (:1190-1194)
            ny = Tl if idx is None else idx.numel()
            part2 = torch.empty(B * Kg, dtype=F32, device=dev)
            H.orca_sim_loss(global16, local16, idx, B, Kg, ny, Tl, h, False, part2)
            out["L_ortho_qformer_local"] = cfg.orca_ortho_weight_qformer_local * part2.sum() / (B * Kg * ny)
        if self.aligns:
            out["L_align_layerwise"] = cfg.orca_align_weight_local * torch.stack([a.mean() for a in self.aligns]).mean()
        return out


# =========================================================================================== causal LM
class CausalLMHIP:
    """Frozen Llama-3.1 / Qwen3 / Qwen2.5 decoder: forward + dX-only backward."""

    def __init__(self, cfg: DeSTA25Config, w: Dict[str, torch.Tensor], device):
        c = cfg.llm_config
        self.c, self.dev = c, device
        self.h, self.L, self.hq, self.hkv, self.hd, self.I, self.V = c.hidden_size, c.num_hidden_layers, c.num_attention_heads, c.num_key_value_heads, c.head_dim, c.intermediate_size, c.vocab_size
        assert self.hd in (64, 128), "head_dim 64 or 128"
        assert self.h % 64 == 0 and self.I % 64 == 0 and (self.hq * self.hd) % 64 == 0
        self.qkvw = (self.hq + 2 * self.hkv) * self.hd
        self.Vp = _r64(self.V)
        dev = device
        check_llm_bias_tensors(c, w.keys() if hasattr(w, "keys") else None)   # (a lazy weight source makes what is asked for: nothing to list)

        def g(name):
            return w[LLM + name].to(dev)

        def T(x):                                   # [out,in] bf16 -> [in, out(+pad)] bf16 via the HIP transpose
            o, i = x.shape
            t = torch.empty(i, _r64(o), dtype=BF16, device=dev)
            H.transpose_to_bf16(x, o, i, t, _r64(o))
            return t
        self._T = T
        self.embed = g("model.embed_tokens.weight").to(BF16).contiguous()
        self.layers = []
        for i in range(self.L):
            p = f"model.layers.{i}."
            wqkv = torch.cat([g(p + "self_attn.q_proj.weight"), g(p + "self_attn.k_proj.weight"), g(p + "self_attn.v_proj.weight")], 0).to(BF16).contiguous()
            wo = g(p + "self_attn.o_proj.weight").to(BF16).contiguous()
            wgu = torch.cat([g(p + "mlp.gate_proj.weight"), g(p + "mlp.up_proj.weight")], 0).to(BF16).contiguous()
            wd = g(p + "mlp.down_proj.weight").to(BF16).contiguous()
            ly = dict(n1=g(p + "input_layernorm.weight").float().contiguous(), n2=g(p + "post_attention_layernorm.weight").float().contiguous(),
                      wqkv=wqkv, wqkvT=T(wqkv), wo=wo, woT=T(wo), wgu=wgu, wd=wd, wdT=T(wd))
            if self.I % 32 == 0:
                # SwiGLU inside the GEMM epilogues (desta_gemm_desc.act 2 / 3): the frozen gate|up rows re-ordered at load into
                # 64-row blocks (32 gate rows, then the 32 matching up rows), so that one wave of the tile kernels owns gate AND up
                # of the same activations.  The plain copy stays for the decode kernels (act 4 walks the concatenated layout);
                # its transpose (the UNFUSED backward, A/B switch) is made on first use.
                if not hasattr(self, "_gu_perm"):
                    b = torch.arange(self.I // 32, device=dev).view(-1, 1) * 32
                    r = torch.arange(32, device=dev).view(1, -1)
                    self._gu_perm = torch.cat([b + r, self.I + b + r], dim=1).reshape(-1)
                ly["wgu_b"] = wgu[self._gu_perm].contiguous()
                ly["wguT_b"] = T(ly["wgu_b"])
            else:
                ly["wguT"] = T(wgu)
            if c.attention_bias:
                # q|k|v projection bias (Qwen2 / Qwen2.5), fp32: the projection GEMMs stay bias-free on every path and the kernel
                # that rotates adds it (`H.rope` / `_kv_append`; rounding rule: DESIGN §3).  The LoRA-merged weight keeps this bias.
                ly["bqkv"] = torch.cat([g(p + f"self_attn.{m}_proj.bias").float() for m in "qkv"]).contiguous()
            if not c.qk_norm and not c.attention_bias and not cfg.use_lora:   # (with adapters the fused-rope path is never taken: no second copy)
                # rotary embedding fused into the q|k|v projection (frozen weights, so a re-layout at load is free): the rows of
                # every q / k head in the order 0, hd/2, 1, hd/2+1, ... put HF's rotate_half pair (i, i + hd/2) on ADJACENT output
                # columns, which one lane of the GEMM epilogue owns; q.k is invariant under a permutation of the head dim applied
                # to both.  A second copy of the weight (+1.6 GB for Llama-3.1-8B): eval / generate keep the plain layout.
                nqk = (self.hq + self.hkv) * self.hd
                il = wqkv.clone()
                il[:nqk] = wqkv[:nqk].view(self.hq + self.hkv, 2, self.hd // 2, wqkv.shape[1]).transpose(1, 2).reshape(nqk, wqkv.shape[1])
                ly["wqkv_il"], ly["wqkvT_il"] = il, T(il)
            if c.qk_norm:
                ly["qn"] = g(p + "self_attn.q_norm.weight").float().contiguous()
                ly["kn"] = g(p + "self_attn.k_norm.weight").float().contiguous()
            self.layers.append(ly)
        self.norm = g("model.norm.weight").float().contiguous()
        self.head = self.embed if c.tie_word_embeddings else g("lm_head.weight").to(BF16).contiguous()
        self.headT = T(self.head)                                             # [h, Vp], zero padded
        self.inv_freq = rope_inv_freq(c).to(dev)
        # A/B switch (bench.py --no-rope-fusion); q/k-norm models (Qwen3) and q|k|v-bias models (Qwen2.5) keep the rope kernel
        self.fuse_rope = not c.qk_norm and not c.attention_bias
        self.B = self.S = 0
        self.lora = None
        self.skip_dead_rows = True                  # A/B switch (bench.py --no-dead-row-skip): last layer on the target tail, layer-0 dX on the audio rows
        self.fuse_swiglu = True                     # A/B switch (bench.py --no-swiglu-fusion): silu(gate) * up and its backward inside the gate|up / d(act) GEMM epilogues
        self.decode_weights = "bf16"                # `set_decode_weights`: what the projections of a KV-cached decode step stream
        self.head8 = self.head4 = None
        self.kv_cache_kind = "bf16"                 # `set_kv_cache`: what generate()'s KV cache holds
        self.kv_cache = self.kv_scale = self.kv_scale_v = None
        self._gen_shape = self._gen_kind = None     # (B, Smax) and cache kind of `_gen_alloc`'s buffers; None = allocate at the next generate()
        self.prefill_chunk = None                   # `set_prefill_chunk`: positions per chunk of generate()'s lean prompt pass; None = `forward`
        self.kv_stage = self._pf = None
        self.speculative = None                     # `set_speculative`: draft tokens per verify step of greedy generate(); None = one token per step
        self.spec_scope = "greedy"                  # `set_speculative(k, scope=...)`: "greedy" = plain greedy calls only, "all" = sampling, penalty and logprobs too
        self.spec_attention = "forward"             # `set_speculative(k, attention=...)`: "forward" = the causal forward kernel, "split" = `H.attention_verify{,_kv8}`
        self._step1 = self._spec = None             # `_step_alloc` sets of the plain step (`_gen_alloc`) and of the verify step (`_spec_alloc`)
        self.spec_stats = None
        self.decode_rows = None                     # `set_decode_rows`: row ceiling of a KV-cached step; None = H.DECODE_MAX_ROWS

    def set_decode_rows(self, n: Optional[int]) -> None:
        """Row ceiling of a KV-cached step (sequences of a plain step, 2 Bc under `guidance_scale`, B (k + 1) of a verify step):
        None or 64 (default) = H.DECODE_MAX_ROWS, what `H.gemm_wide` takes; an int in 65..H.DECODE_TALL_MAX_ROWS lets steps of more
        than 64 rows run, their projections through `H.gemm_tall` on bf16 or FP8 decode weights (one weight pass per step whatever
        the rows; MXFP4 decode weights stay at 64 rows and say so).  Steps of at most 64 rows run what they ran before.  Above 64
        sequences the prompt pass is the lean `prefill`, in chunks of `tall_prefill_chunk(B)` positions unless `set_prefill_chunk`
        names a size."""
        check_decode_rows_arg(n)
        self.decode_rows = None if n in (None, H.DECODE_MAX_ROWS) else n

    decode_rows: Optional[int] = None               # (class defaults: the settings of a model nobody has set)
    decode_weights: str = "bf16"

    @property
    def row_limit(self) -> int:
        """Rows a KV-cached step of this model takes: `set_decode_rows`, or H.DECODE_MAX_ROWS by default and with MXFP4 decode
        weights, which have no kernel above it."""
        return H.DECODE_MAX_ROWS if self.decode_weights == "mxfp4" else (self.decode_rows or H.DECODE_MAX_ROWS)

    def check_rows(self, B: int, guided: bool = False) -> None:
        """`check_decode_rows` at this model's ceiling; under MXFP4 decode weights the rows `set_decode_rows` would admit say so."""
        if self.decode_weights == "mxfp4" and H.DECODE_MAX_ROWS < B <= (self.decode_rows or H.DECODE_MAX_ROWS):
            raise ValueError(f"generate: {B} rows in a KV-cached step with MXFP4 decode weights: `gemm_w4` takes at most {H.DECODE_MAX_ROWS} "
                             f"(`set_decode_rows` covers bf16 and FP8 decode weights): split the batch or set another weight kind")
        check_decode_rows(B, guided, self.row_limit)

    def _prompt_chunk(self, B: int) -> Optional[int]:
        """Positions per chunk of generate()'s prompt pass for B rows: `set_prefill_chunk`, else `tall_prefill_chunk` (None = `forward`)."""
        return self.prefill_chunk if self.prefill_chunk is not None else tall_prefill_chunk(B)

    def set_speculative(self, k: Optional[int], scope: str = "greedy", attention: str = "forward") -> None:
        """generate(): None or 0 (default) = one token per sequence per pass over the weights; an int k in 1..7 = draft and
        verify: k tokens proposed by looking the row's last tokens up in its own prompt and output (`H.spec_ngram_draft`), all k + 1
        rows per sequence checked by ONE pass (`verify_step`: the step body of `decode_step`, `_step_rows`, at width k + 1), and
        the longest run every unfinished row agrees on is emitted (`H.spec_accept`; acceptance is in lockstep, so the cache keeps
        one length).  The tokens are those of the plain loop up to the rounding of a different row count.
        scope = "greedy" (default): only plain greedy calls speculate; sampling, a repetition penalty and `logprobs` run the plain
        loop.  scope = "all": those three speculate too.  Row j of a sequence is picked by the sampler the plain loop would launch
        for emitted position n + j, with that position's RNG counter and token history (`H.sample_rows`, `H.sample_top_p_rows`), so
        the token is the sampler's own draw from the logits of the accepted prefix and a draft is accepted exactly when the draw
        hits it: the plain loop's sampled tokens, with no rejection-resampling rule.  `logprobs` costs one `H.topk_logprobs` launch
        over all rows per verify step.
        attention = "forward" (default): a verify step attends through the causal forward kernel at seq_q = k + 1, one block per
        query head walking the whole cache.  attention = "split": through the split-KV verify kernels (`H.attention_verify`,
        `H.attention_verify_kv8`: K / V once for all G (k + 1) query rows of a KV head, a row's 256-key chunks on different CUs).
        On the bf16 cache iff head_dim is 128, G <= 8, G (k + 1) <= H.VERIFY_ATTN_MAX_ROWS and cur + 1 >= H.DECODE_ATTN_MIN_KEYS, the
        plain loop's own rule at the step's first row (the forward kernel otherwise); row j of that kernel is the plain step's
        split-KV result at slot cur + j bit for bit, so from that slot on both loops run one attention arithmetic.  On the FP8 KV
        cache, where only "split" speculates, at every cur.
        Under both scopes `forced_tokens`, a `layer_hook` (ORCA), B * (k + 1) > `row_limit` (H.DECODE_MAX_ROWS, or `set_decode_rows`) and the FP8 KV cache (with
        attention = "forward", or with more than H.VERIFY_ATTN_MAX_ROWS query rows per KV head) run the plain loop; `spec_stats`
        says which ran and why."""
        check_speculative_arg(k)
        check_speculative_scope(scope)
        check_speculative_attention(attention)
        k = k or None
        if k != self.speculative:                                            # the verify buffers go with k, not with the scope or the attention
            self._spec = None
        self.speculative = k
        self.spec_scope = scope
        self.spec_attention = attention

    def set_prefill_chunk(self, n: Optional[int]) -> None:
        """Prompt pass of generate(): None (default) = the training `forward` with its per-layer save set; an int >= 16 = the
        lean `prefill`, which walks the prompt in chunks of n positions on rolling buffers shared by every layer and chunk, each
        chunk attending the KV cache the earlier ones filled (n >= the prompt: one chunk).  Memory outside the cache then follows
        n, not the prompt length or the layer count.  Under the FP8 cache a chunk attends every key, its own included, as the
        decode steps will see it (dequantised e4m3); `forward` attends the bf16 projection."""
        check_prefill_chunk(n)
        if n != self.prefill_chunk:                                          # the chunk buffers (and the FP8 staging slab) go with the setting
            self._pf = self.kv_stage = None
            self._gen_shape = None
        self.prefill_chunk = n

    # -- weight-only FP8 (e4m3) decode: a second, half-size copy of the frozen decode-side weights -------------------------------
    DECODE_WEIGHT_KINDS = ("bf16", "fp8")
    DECODE_WEIGHT_KINDS_MX = ("mxfp4",)             # block-scaled kinds: OCP MXFP4 (e2m1 nibbles, one e8m0 scale per 32 k)

    def set_decode_weights(self, kind: str) -> None:
        """What `decode_step` streams: "bf16" (default, the reference's arithmetic), "fp8" = OCP e4m3 bytes with one power-of-two
        scale per output row (W8A16) or "mxfp4" = OCP e2m1 nibbles with one e8m0 scale per 32 consecutive k (W4A16, round to
        nearest, no calibration); activations, KV cache and accumulation unchanged.  The copies are made at the first decode step
        that needs them; "bf16" frees both sets, "fp8" and "mxfp4" free each other's.  The prompt pass and training always use the
        bf16 weights."""
        kinds = self.DECODE_WEIGHT_KINDS + self.DECODE_WEIGHT_KINDS_MX
        if kind not in kinds:
            raise ValueError(f"decode_weights must be one of {kinds}, got {kind!r}")
        self.decode_weights = kind
        if kind != "fp8":
            self.head8 = None
            for ly in self.layers:
                ly.pop("q8", None)
        if kind != "mxfp4":
            self.head4 = None
            for ly in self.layers:
                ly.pop("q4", None)

    # -- FP8 (e4m3) KV cache: bytes + one power-of-two scale per (row, slot, K-or-V head) (include/desta_hip.h) ------------------
    KV_CACHE_KINDS = ("bf16", "fp8")

    def set_kv_cache(self, kind: str) -> None:
        """What generate()'s KV cache holds: "bf16" (default, the reference's arithmetic) or "fp8" = OCP e4m3 bytes, quantised
        per head where a token is appended and dequantised in registers where the decode attention reads it (0.516 of the bf16
        bytes).  The prompt pass's own attention reads the bf16 q|k|v projection either way, so prompt logits do not depend on
        the kind.  "fp8" needs the split-KV decode kernel's geometry: head_dim 128 and at most 8 query heads per KV head.  With
        `set_speculative(k)` the FP8 cache speculates only under `attention="split"` and G (k + 1) <= H.VERIFY_ATTN_MAX_ROWS query rows
        per KV head (the verify kernel that reads the bytes); otherwise the plain loop runs and `spec_stats` says why."""
        if kind not in self.KV_CACHE_KINDS:
            raise ValueError(f"kv_cache must be one of {self.KV_CACHE_KINDS}, got {kind!r}")
        if kind == "fp8" and (self.hd != 128 or self.hq // self.hkv > 8):
            raise ValueError(f"kv_cache 'fp8' needs head_dim 128 and at most 8 query heads per KV head, got head_dim {self.hd}, "
                             f"{self.hq // self.hkv} per KV head")
        if kind != self.kv_cache_kind:                                       # the other kind's slabs are freed; `_gen_alloc` makes the new ones
            self.kv_cache = self.kv_scale = self.kv_scale_v = self.kv_stage = None
            self._gen_shape = None
        self.kv_cache_kind = kind

    def _fp8_decode_weights(self) -> None:
        """Quantise once: q|k|v, o, gate|up (the concatenated decode copy) and down of every layer, and the lm_head (tied
        embeddings: the bf16 table stays for the gather).  With adapters the q|k|v projection is left out: its merged weight
        changes with training."""
        if self.head8 is not None:
            return
        names = ("wo", "wgu", "wd") if self.lora is not None else ("wqkv", "wo", "wgu", "wd")
        for ly in self.layers:
            ly["q8"] = {n: H.quantize_rows_e4m3(ly[n]) for n in names}
        self.head8 = H.quantize_rows_e4m3(self.head)

    def _mxfp4_decode_weights(self) -> None:
        """`_fp8_decode_weights` for "mxfp4": (nibbles [rows, K / 2], e8m0 scales [rows, K / 32]) of the same weights into ly["q4"]
        and `head4`; with adapters the q|k|v projection stays bf16."""
        if self.head4 is not None:
            return
        names = ("wo", "wgu", "wd") if self.lora is not None else ("wqkv", "wo", "wgu", "wd")
        for ly in self.layers:
            ly["q4"] = {n: H.quantize_rows_mxfp4(ly[n]) for n in names}
        self.head4 = H.quantize_rows_mxfp4(self.head)
    # -- LoRA adapters on q/k/v (reference: peft, modeling_desta25.py:720-729; published layer: y = W x + (alpha / r) B A drop(x)) --------
    LORA_KP = 64                                    # the three rank-r adapters side by side, padded to one 64-wide GEMM K block

    def attach_lora(self, arena: ParamArena, r: int, alpha: float, p_drop: float) -> None:
        """The adapters live in the trainable arena (fp32, like peft keeps them); `refresh_lora` makes the bf16 operand copies:
        per layer `a16` [64, h] (rows 16p..16p+r = A_p, the rest zero), `b16` [(Hq+2Hkv) hd, 64] block-diagonal (rows of
        projection p carry scaling * B_p in columns 16p..16p+r), so that  t = x a16^T  [M, 64]  and  qkv += t b16^T  are two
        GEMMs for all three projections.  The rows in front of the first audio span cannot be skipped in the backward (their
        keys / values carry adapter gradient), and the rotary embedding stays a separate kernel (it follows the adapter sum)."""
        assert 3 * r <= self.LORA_KP
        self.lora = dict(arena=arena, r=r, scaling=alpha / r, p=p_drop, dirty=True, merged_dirty=True, seed_base=0, p_now=0.0)
        h, dev = self.h, self.dev
        for ly in self.layers:
            ly["a16"] = torch.zeros(self.LORA_KP, h, dtype=BF16, device=dev)
            ly["b16"] = torch.zeros(self.qkvw, self.LORA_KP, dtype=BF16, device=dev)
            ly["a16p"] = [torch.zeros(self.LORA_KP, h, dtype=BF16, device=dev) for _ in LORA_TARGETS]   # a16 with the rows of ONE projection (dropout backward)
            # the pair-interleaved q|k|v copies only serve the fused rotary epilogue, which the adapter sum rules out (`forward`): free them
            ly.pop("wqkv_il", None)
            ly.pop("wqkvT_il", None)
        self.B = self.S = 0                                                    # re-allocate the activations with the adapter buffers

    def _lora_names(self, i: int, ab: str) -> List[str]:
        return [f"{LLM}model.layers.{i}.self_attn.{m}_proj.lora_{ab}.default.weight" for m in LORA_TARGETS]

    def refresh_lora(self) -> None:
        lo = self.lora
        if lo is None or not lo["dirty"]:
            return
        r, ar = lo["r"], lo["arena"]
        outs = (self.hq * self.hd, self.hkv * self.hd, self.hkv * self.hd)
        for i, ly in enumerate(self.layers):
            row = 0
            for j, (na, nb) in enumerate(zip(self._lora_names(i, "A"), self._lora_names(i, "B"))):
                ly["a16"][16 * j:16 * j + r].copy_(ar.param(na))
                ly["a16p"][j][16 * j:16 * j + r].copy_(ar.param(na))
                ly["b16"][row:row + outs[j], 16 * j:16 * j + r].copy_(ar.param(nb) * lo["scaling"])
                row += outs[j]
        lo["dirty"], lo["merged_dirty"] = False, True

    def _lora_merged(self, i: int) -> torch.Tensor:
        """q|k|v weight with the adapters merged, W + scaling * B A (bf16), for generate(): the decode kernels stream ONE weight."""
        lo = self.lora
        if lo["merged_dirty"]:
            for ly in self.layers:
                if "wqkv_m" not in ly:
                    ly["wqkv_m"] = torch.empty_like(ly["wqkv"])
                H.gemm(ly["b16"], ly["a16"], ly["wqkv_m"], self.qkvw, self.h, self.LORA_KP, trans_b=True, ldb=self.h, residual=ly["wqkv"])
            lo["merged_dirty"] = False
        return self.layers[i]["wqkv_m"]

    def _lora_seed(self, i: int, j: int) -> int:
        return site_seed(self.lora["seed_base"], 2, i, j)                    # domain 2: apart from the Q-Former's sites (domain 1) of any forward

    def _lora_fwd(self, i: int, ly, s, M: int) -> None:
        """s["qkv"] (plain layout, before the rotary embedding) += adapters of layer i applied to self.hb."""
        lo, h, KP = self.lora, self.h, self.LORA_KP
        tT = s["lt"]                                                             # t^T [64, Mp]: rows 16p.. = A_p drop_p(x)^T
        for j in range(len(LORA_TARGETS)):
            xin = self.hb
            if lo["p_now"] > 0.0:                                                # peft: every adapted module has its OWN dropout
                xin = s["lxd"][j]                                                # kept for the backward's dA (3 x [M, h] bf16 per layer)
                H.dropout_bf16(self.hb, xin, M, h, h, lo["p_now"], self._lora_seed(i, j))
            # 16 output rows: the weight-streaming (decode) kernel, with the TOKENS as its streamed operand (x is read at HBM
            # rate; as t = x A^T with N = 16 the tile kernel ran 40 blocks at 0.7 TB/s)
            H.gemm(ly["a16"][16 * j:16 * j + 16], xin, tT[16 * j:16 * j + 16], 16, self.Mp, h, ldc=self.Mp)
        Mg = M if M % 8 == 0 else self.Mp                                         # transposed-storage A wants a multiple of 8 rows: the pad rows of t^T are zero, q|k|v has Mp rows
        H.gemm(tT, ly["b16"], s["qkv"], Mg, self.qkvw, KP, trans_a=True, lda=self.Mp, residual=s["qkv"])

    def _lora_bwd(self, i: int, ly, s, dhb, M: int) -> None:
        """Adapter gradients of layer i into the arena, and dhb [M, h] += their input gradient.  self.dqkv = d(q|k|v) of the
        plain layout, all M rows; the reduction over tokens runs on Mp = M rounded up to 64 rows whose pad rows are zero."""
        lo, h, KP, Mp = self.lora, self.h, self.LORA_KP, self.Mp
        ar, r = lo["arena"], lo["r"]
        t, dt = s["lt"], self.ldt
        if lo["p_now"] <= 0.0:
            H.rmsnorm_fwd(self.xs[i], ly["n1"], self.c.rms_norm_eps, self.lhb, self.lr1)       # the projection's input again (not kept by the forward)
        outs = (self.hq * self.hd, self.hkv * self.hd, self.hkv * self.hd)
        col = 0
        for j, nb in enumerate(self._lora_names(i, "B")):                                      # dB_p = scaling * dY_p^T t_p
            H.gemm(self.dqkv[:, col:], t[16 * j:16 * j + 16], ar.grad(nb), outs[j], r, Mp, trans_a=True, lda=self.qkvw, ldb=Mp, alpha=lo["scaling"])
            col += outs[j]
        H.gemm(self.dqkv, ly["b16"], dt, M, KP, self.qkvw, trans_b=True, ldb=KP)                # dt = dY (scaling B)
        na = self._lora_names(i, "A")
        if lo["p_now"] > 0.0:
            for j in range(len(LORA_TARGETS)):
                H.gemm(dt[:, 16 * j:], s["lxd"][j], ar.grad(na[j]), r, h, Mp, trans_a=True, trans_b=True, lda=KP, ldb=h)
                # dhb += drop_p'(dt_p A_p): the mask and the accumulation ride in the GEMM's epilogue (element index m * h + n, as forward)
                H.gemm(dt, ly["a16p"][j], dhb, M, h, KP, trans_b=True, ldb=h, residual=dhb, dropout_p=lo["p_now"], dropout_seed=self._lora_seed(i, j))
        else:
            ga = ar.grads[ar.offsets[na[0]]:ar.offsets[na[0]] + 3 * r * h].view(3 * r, h) if r == 16 else None
            if ga is not None:
                H.gemm(dt, self.lhb, ga, 3 * r, h, Mp, trans_a=True, trans_b=True, lda=KP, ldb=h)
            else:
                for j in range(len(LORA_TARGETS)):
                    H.gemm(dt[:, 16 * j:], self.lhb, ar.grad(na[j]), r, h, Mp, trans_a=True, trans_b=True, lda=KP, ldb=h)
            H.gemm(dt, ly["a16"], dhb, M, h, KP, trans_b=True, ldb=h, residual=dhb)

    def _b16(self, *shape) -> torch.Tensor:
        return torch.empty(*shape, dtype=BF16, device=self.dev)

    def _alloc(self, B: int, S: int):
        h, dev, M, b16 = self.h, self.dev, B * S, self._b16
        self.B, self.S, self.M = B, S, M
        fr = torch.outer(torch.arange(S, device=dev, dtype=F32), self.inv_freq)
        self.cos_sin = torch.stack([fr.cos(), fr.sin()], dim=1).contiguous()                 # [S, 2, hd/2]
        self.cos_sin_il = torch.stack([fr.cos(), fr.sin()], dim=2).contiguous()              # [S, hd/2, 2]: (cos, sin) per adjacent pair
        ar = torch.arange(M, device=dev, dtype=torch.int32)
        self.pos_rows = {False: (ar % S).contiguous(), True: (ar // B).contiguous()}         # position of a token row: batch-major / position-major
        self.xs = [b16(M, h) for _ in range(self.L + 1)]
        self.sv = []
        for _ in range(self.L):
            s = dict(r1=torch.empty(M, dtype=F32, device=dev), qkv=b16(M, self.qkvw), att=b16(M, self.hq * self.hd),
                     lse=torch.empty(B, self.hq, S, dtype=F32, device=dev), xm=b16(M, h), r2=torch.empty(M, dtype=F32, device=dev), gu=b16(M, 2 * self.I))
            if self.c.qk_norm:
                s["pre"] = b16(M, self.qkvw)
            self.sv.append(s)
        self.rf = torch.empty(M, dtype=F32, device=dev)
        self.hb = torch.zeros(_r64(M), h, dtype=BF16, device=dev)                           # (rows >= M stay zero: the adapters' token-streaming GEMM reads whole 64-row groups)
        self.hbc = b16(M, h)                                                                 # compact target rows (lm_head in / dX out)
        self.act = b16(M, self.I)
        self.logits = torch.zeros(M, self.Vp, dtype=BF16, device=dev)                        # pad columns stay 0
        self.loss = torch.zeros(1, dtype=F32, device=dev)
        # backward scratch
        self.dxa, self.dxb = b16(M, h), b16(M, h)
        self.dgu = b16(M, 2 * self.I)
        self.Mp = _r64(M)
        self.dqkv = torch.zeros(self.Mp, self.qkvw, dtype=BF16, device=dev)                  # rows >= M: zero (token-reduction operand of the adapter gradients)
        self.datt = torch.zeros(M, self.hq * self.hd, dtype=BF16, device=dev)                # rows in front of the first audio span stay 0
        if self.lora is not None:
            # token-reduction operands of the adapter gradients: Mp rows, pad rows zero for good (kernels write rows < M only)
            z = lambda *sh: torch.zeros(*sh, dtype=BF16, device=dev)
            self.lhb, self.ldt = z(self.Mp, h), z(self.Mp, self.LORA_KP)
            self.lr1 = torch.empty(M, dtype=F32, device=dev)
            for s in self.sv:
                s["lt"] = z(self.LORA_KP, self.Mp)                             # t^T
                s["qkv"] = z(self.Mp, self.qkvw)                               # (Mp rows: see `_lora_fwd`)
                if self.lora["p"] > 0.0:
                    s["lxd"] = [z(self.Mp, h) for _ in LORA_TARGETS]         # the three dropped inputs of the layer (training)

    def forward(self, x0_filler, B: int, S: int, kv_start: Optional[torch.Tensor], labels: Optional[torch.Tensor], need_grad: bool,
                pos_shift: Optional[torch.Tensor] = None, cos_sin: Optional[torch.Tensor] = None, last_logits: Optional[torch.Tensor] = None,
                kv_cache: Optional[List[torch.Tensor]] = None, target_rows=None, s_major: bool = False, layer_hook=None):
        """`x0_filler(buf)` writes inputs_embeds [B*S, h] bf16 into buf.  Returns the logits buffer [B*S, Vp].
        Training uses position_ids = arange(S) (H7); generate() passes pos_shift (= -left_pad per sequence, with a
        `cos_sin` table that also covers the new tokens), `last_logits` [B, Vp] to project only the last row, and the
        per-layer KV cache slabs that the rope kernel fills with the prompt's keys / values."""
        if (B, S) != (self.B, self.S):
            self._alloc(B, S)
        c, h, M = self.c, self.h, self.M
        x0_filler(self.xs[0])
        self.kv_start = kv_start
        scale = self.hd ** -0.5
        cs = self.cos_sin if cos_sin is None else cos_sin
        # s_major (training): row = s * B + b, so "all positions >= s0" is ONE contiguous row range and the backward can
        # skip the rows in front of the first audio span; per-sequence kernels then see row stride B*width, batch stride width
        self.s_major = bool(s_major)
        smb = B if s_major else 0
        rsm = B if s_major else 1
        # rotary embedding inside the q|k|v GEMM epilogue: training / eval forward over a whole sequence with arange positions
        # (H7); the backward then needs the 8-wave dQ path (seq >= 128).  generate() (cache append, shifted positions) and
        # q/k-norm models keep the separate kernel.
        fused = self._rope_fused = bool(self.fuse_rope and "wqkv_il" in self.layers[0] and kv_cache is None and pos_shift is None
                                        and cos_sin is None and S >= 128 and M > 16 and self.lora is None)
        lora = self.lora is not None and kv_cache is None                 # generate(): merged weights instead (`_lora_merged`)
        if self.lora is not None:
            self.refresh_lora()
            self.lora["p_now"] = self.lora["p"] if need_grad else 0.0
        # rows of the LAST layer's output that anything reads: with the compact lm_head only the target rows, which in the
        # position-major grid are the contiguous tail [first target position * B, M) (left padding aligns every sequence's end).
        # o_proj, the MLP and the final norm of the last layer run on that tail only (its attention still sees every key).
        self.tail0 = 0
        for i, (ly, s) in enumerate(zip(self.layers, self.sv)):
            x = self.xs[i]
            if i == self.L - 1 and target_rows is not None and self.s_major and self.skip_dead_rows and self.L > 1:
                target_rows[3].synchronize()                                   # side stream of `_target_rows`: long done
                self.tail0 = min(int(target_rows[2][1]), S) * B
            H.rmsnorm_fwd(x, ly["n1"], c.rms_norm_eps, self.hb, s["r1"])
            if fused:
                H.gemm(self.hb, ly["wqkv_il"], s["qkv"], M, self.qkvw, h,
                       rope=(self.cos_sin_il, self.pos_rows[self.s_major], (self.hq + self.hkv) * self.hd, self.hd))
            elif lora:
                H.gemm(self.hb, ly["wqkv"], s["qkv"], M, self.qkvw, h)
                self._lora_fwd(i, ly, s, M)
                if "pre" in s:
                    s["pre"].copy_(s["qkv"][:M])                              # q/k-norm backward wants the projection before the norm
            else:
                H.gemm(self.hb, ly["wqkv"] if self.lora is None else self._lora_merged(i), s["qkv"], M, self.qkvw, h, preact=s.get("pre"))
            if fused:
                pass                                                          # q, k left the projection rotated
            elif kv_cache is None:
                H.rope(s["qkv"], self.qkvw, M, S, self.hq, self.hkv, self.hd, cs, ly.get("qn"), ly.get("kn"), c.rms_norm_eps, pos_shift=pos_shift,
                       s_major_batch=smb, **({"bias": ly["bqkv"]} if "bqkv" in ly else {}))
            else:                                                             # generate(): `kv_cache` is self.kv_cache, `cos_sin` its table
                self._kv_append(i, ly, s["qkv"], M, S, pos_shift, 0)
            aw = self.hq * self.hd
            ad = H.attn_desc(s["qkv"], s["qkv"], s["qkv"], s["att"], s["lse"], batch=B, hq=self.hq, hkv=self.hkv, sq=S, sk=S, hd=self.hd,
                             scale=scale, causal=True, kv_start=kv_start, q_off=0, k_off=self.hq * self.hd, v_off=(self.hq + self.hkv) * self.hd,
                             q_rs=rsm * self.qkvw, k_rs=rsm * self.qkvw, v_rs=rsm * self.qkvw, o_rs=rsm * aw,
                             q_bs=self.qkvw if s_major else None, k_bs=self.qkvw if s_major else None,
                             v_bs=self.qkvw if s_major else None, o_bs=aw if s_major else None)
            H.attention_fwd(ad)
            s["ad"] = ad
            t0 = self.tail0 if i == self.L - 1 else 0
            Mt = M - t0
            if Mt > 0:
                H.gemm(s["att"][t0:], ly["wo"], s["xm"][t0:], Mt, h, self.hq * self.hd, residual=x[t0:])
                H.rmsnorm_fwd(s["xm"][t0:], ly["n2"], c.rms_norm_eps, self.hb[t0:], s["r2"][t0:])
                s["gu_blocked"] = self.fuse_swiglu and "wgu_b" in ly
                if s["gu_blocked"]:
                    # one launch: the projection (kept for the backward, 64-column gate|up blocks) and silu(gate) * up
                    H.gemm(self.hb[t0:], ly["wgu_b"], s["gu"][t0:], Mt, 2 * self.I, h, act=2, aux=self.act[t0:], ld_aux=self.I)
                else:
                    H.gemm(self.hb[t0:], ly["wgu"], s["gu"][t0:], Mt, 2 * self.I, h)
                    H.swiglu_fwd(s["gu"][t0:], self.act[t0:], Mt, self.I)
                H.gemm(self.act[t0:], ly["wd"], self.xs[i + 1][t0:], Mt, h, self.I, residual=s["xm"][t0:])
            if layer_hook is not None:                                        # ORCA deep injection: the wrapped decoder layer's output (batch-major grid)
                layer_hook(i, self.xs[i + 1])
        t0 = self.tail0
        if M - t0 > 0:
            H.rmsnorm_fwd(self.xs[self.L][t0:], self.norm, c.rms_norm_eps, self.hb[t0:], self.rf[t0:])
        if last_logits is not None:                      # rows b*S + S-1 only: A is a strided view of hb
            H.gemm(self.hb[S - 1:], self.head, last_logits, B, self.V, h, lda=S * h, ldc=self.Vp)
            return last_logits
        self.compact = None
        if target_rows is not None:
            # training without returned logits: lm_head / CE / lm_head backward only on the rows that carry a target
            # (ForCausalLMLoss ignores the others; their gradient is exactly zero).  The row count comes from a side stream
            # that only depends on `labels`, so waiting for it here does not drain the main stream.
            idx, lab_c, count_host, ev = target_rows
            ev.synchronize()
            Mc = int(count_host[0])
            if Mc > 0:
                H.gather_rows(self.hb, idx, Mc, h, self.hbc)
                H.gemm(self.hbc, self.head, self.logits, Mc, self.V, h, ldc=self.Vp)        # compact logits in rows [0, Mc)
            self.compact = (idx, lab_c, Mc)                                                  # Mc == 0: no target in the batch
            return self.logits
        H.gemm(self.hb, self.head, self.logits, M, self.V, h, ldc=self.Vp)
        return self.logits

    # -- greedy decoding with a KV cache (reference: llm_model.generate, modeling_desta25.py:1419) ------
    def _gen_alloc(self, B: int, Smax: int):
        if self._gen_shape == (B, Smax) and self._gen_kind == self.kv_cache_kind:
            return
        dev, b16 = self.dev, self._b16
        self._gen_shape, self._gen_kind = (B, Smax), self.kv_cache_kind
        self.kvw = 2 * self.hkv * self.hd
        # one [B, Smax, K|V] slab per layer: a decode step reads keys/values with row stride kvw, batch stride Smax*kvw
        self.kv_cache = self.kv_scale = self.kv_scale_v = self.kv_stage = self._step1 = None     # free the old slabs before the new ones are made
        if self.kv_cache_kind == "fp8":                                      # e4m3 bytes + fp32 scales [B, Smax, K heads | V heads]
            self.kv_cache = [torch.empty(B, Smax, self.kvw, dtype=torch.uint8, device=dev) for _ in range(self.L)]
            self.kv_scale = [torch.empty(B, Smax, 2 * self.hkv, dtype=F32, device=dev) for _ in range(self.L)]
            self.kv_scale_v = [sc[:, :, self.hkv:] for sc in self.kv_scale]
            # chunked prompt pass: ONE layer's slots as bf16 for the forward kernel (`prefill`), 1 / L of a bf16 cache.  Zeroed: the
            # dequantisation leaves the slots in front of kv_start alone, and the forward kernel multiplies the V rows of a masked
            # key of the first visible tile by p = 0, so they have to be finite (in the bf16 cache the append writes them)
            self.kv_stage = torch.zeros(B, Smax, self.kvw, dtype=BF16, device=dev) if self._prompt_chunk(B) is not None else None
        else:
            self.kv_cache = [b16(B, Smax, self.kvw) for _ in range(self.L)]
        fr = torch.outer(torch.arange(Smax, device=dev, dtype=F32), self.inv_freq)
        self.gen_cos_sin = torch.stack([fr.cos(), fr.sin()], dim=1).contiguous()
        self._step1 = self._step_alloc(B, 1)                                 # one row per sequence; its logits also take the prompt pass's last row
        # fp32 chunk partials of the split-KV decode attention, sized once for the longest cache (0 bytes while it fits one chunk)
        ws = H.attention_decode_workspace_bytes(B, self.hq, Smax, self.hd) if self.hd == 128 and self.hq // self.hkv <= 8 else 0
        self.g_attn_ws = torch.empty(ws // 4, dtype=F32, device=dev) if ws else None
        self.g_next = torch.zeros(B, dtype=torch.int64, device=dev)

    def _step_alloc(self, B: int, w: int) -> dict:
        """Activations of one KV-cached step (`_step_rows`) over M = B * w rows, batch-major with w rows per sequence."""
        h, dev, b16, M = self.h, self.dev, self._b16, B * w
        return dict(x=b16(M, h), xm=b16(M, h), hb=b16(M, h), qkv=b16(M, self.qkvw), att=b16(M, self.hq * self.hd),
                    lse=torch.empty(B, self.hq, w, dtype=F32, device=dev), act=b16(M, self.I), r=torch.empty(M, dtype=F32, device=dev),
                    logits=torch.zeros(M, self.Vp, dtype=BF16, device=dev))     # pad columns stay 0

    def _kv_append(self, li: int, ly: dict, qkv: torch.Tensor, rows: int, seq: int, shift: torch.Tensor, slot0: int) -> None:
        """Rotate q, k of `qkv` [rows, qkvw] (batch-major, `seq` rows per sequence, position = row's index + shift[b]) in place and
        append the rotated K | V of layer `li` at slots [slot0, slot0 + seq) of its cache slab.  The slab's dtype picks the kernel:
        bf16 as it is, uint8 (FP8 cache) quantised per head with the scales into `kv_scale[li]`.  Every stride is the tensor's.
        A q|k|v bias (`bqkv`) is added by the same kernel in front of the rotation, so no caller has a branch for it."""
        cache = self.kv_cache[li]
        bias = {"bias": ly["bqkv"]} if "bqkv" in ly else {}                   # bias-free models make the call they always made
        args = (qkv, self.qkvw, rows, seq, self.hq, self.hkv, self.hd, self.gen_cos_sin, ly.get("qn"), ly.get("kn"), self.c.rms_norm_eps, shift,
                cache, cache.stride(0), cache.stride(1))
        if cache.dtype == torch.uint8:
            sc = self.kv_scale[li]
            H.rope_kv_append_e4m3(*args, sc, sc.stride(0), sc.stride(1), slot0, **bias)
        else:
            H.rope_kv_append(*args, slot0, **bias)

    def _cache_attn_desc(self, qkv: torch.Tensor, slab: torch.Tensor, att: torch.Tensor, lse: torch.Tensor, B: int, sq: int, sk: int, causal: bool,
                         kv_start: torch.Tensor, **strides):
        """Attention of `sq` query rows per sequence over slots [kv_start, sk) of a cache slab: Q the first columns of `qkv`
        [B * sq, qkvw] (batch-major), K | V the halves of `slab` [B, Smax, kvw] (a layer's cache, or `kv_stage`), O into `att`.
        causal: the mask "key <= query + (sk - sq)"."""
        qkvw, kvw, bs = self.qkvw, self.kvw, slab.stride(0)
        return H.attn_desc(qkv, slab, slab, att, lse, batch=B, hq=self.hq, hkv=self.hkv, sq=sq, sk=sk, hd=self.hd, scale=self.hd ** -0.5,
                           causal=causal, kv_start=kv_start, q_off=0, k_off=0, v_off=self.hkv * self.hd, q_rs=qkvw, k_rs=kvw, v_rs=kvw,
                           o_rs=self.hq * self.hd, k_bs=bs, v_bs=bs, **strides)

    # -- lean, chunked prompt pass of generate() (`set_prefill_chunk`): nothing is kept for a backward ---------------------------
    def _prefill_alloc(self, B: int, S: int, Cm: int) -> dict:
        """Buffers of `prefill`: the prompt's embeddings [B*S, h] (the only one sized by S) and ONE set of per-chunk activations
        for B * Cm rows, shared by every layer and chunk."""
        pf = self._pf
        if pf is not None and pf["key"] == (B, S, Cm):
            return pf
        self._pf = pf = None                                                 # free the old set before the new one is made
        h, dev, M, b16 = self.h, self.dev, B * Cm, self._b16
        self._pf = pf = dict(key=(B, S, Cm), x0=b16(B * S, h), xa=b16(M, h), xb=b16(M, h), hb=b16(M, h), qkv=b16(M, self.qkvw),
                             att=b16(M, self.hq * self.hd), xm=b16(M, h), gu=b16(M, 2 * self.I), act=b16(M, self.I),
                             lse=torch.empty(B * self.hq * Cm, dtype=F32, device=dev), r=torch.empty(M, dtype=F32, device=dev))
        return pf

    def prefill(self, x0_filler, B: int, S: int, kv_start: torch.Tensor, last_logits: torch.Tensor, layer_hook=None, chunk_hook=None) -> torch.Tensor:
        """The prompt pass of generate() without a save set (needs `_gen_alloc` and a chunk size): `x0_filler(buf)` writes
        inputs_embeds [B*S, h]; the prompt is walked in the chunks of `prefill_chunks(S, self.prefill_chunk)`.  A chunk [c0, c1) of
        every sequence runs through all layers with the kernels, weight forms and switches of `forward`'s generate() branch
        (unfused q|k|v projection, the adapters merged, blocked gate|up + SwiGLU epilogue when `fuse_swiglu`; the copy of the
        projection in front of the q/k-norm is a backward operand and is not made), appends its rotated K | V at slots [c0, c1)
        (position = slot - left pad) and attends slots [kv_start, c1) of the layer's cache slab under the causal mask
        "key <= query + (seq_k - seq_q)".  FP8 cache: the slots up to c1 are dequantised into the one staging slab first, so
        every key, the chunk's own included, is the value the decode steps will read.  After the last chunk the last row of each
        sequence is projected into `last_logits` [B, Vp].  `chunk_hook(i, Cc)` runs in front of chunk i (ORCA sizes its row
        buffers), `layer_hook(l, x)` behind every layer on the chunk's rows [B*Cc, h] (batch-major)."""
        c, h, hq, hkv, hd = self.c, self.h, self.hq, self.hkv, self.hd
        chunks = prefill_chunks(S, self._prompt_chunk(B))
        pf = self._prefill_alloc(B, S, chunks[0][1])
        Smax, kvw, aw, eps = self._gen_shape[1], self.kvw, hq * hd, c.rms_norm_eps
        kv8 = self._gen_kind == "fp8"
        x0_filler(pf["x0"])
        x0 = pf["x0"].view(B, S, h)
        if self.lora is not None:
            self.refresh_lora()
        blocked = self.fuse_swiglu and "wgu_b" in self.layers[0]
        for ci, (c0, c1) in enumerate(chunks):
            Cc = c1 - c0
            M = B * Cc
            x, y, hb, qkv, att, xm, gu, act, r = (pf[k][:M] for k in ("xa", "xb", "hb", "qkv", "att", "xm", "gu", "act", "r"))
            lse = pf["lse"][:B * hq * Cc].view(B, hq, Cc)
            x.view(B, Cc, h).copy_(x0[:, c0:c1])                              # the chunk's rows, batch-major
            shift = (c0 - kv_start).to(torch.int32).contiguous()             # position of the chunk's row j: c0 + j - left pad
            if chunk_hook is not None:
                chunk_hook(ci, Cc)
            for i, ly in enumerate(self.layers):
                H.rmsnorm_fwd(x, ly["n1"], eps, hb, r)
                H.gemm(hb, ly["wqkv"] if self.lora is None else self._lora_merged(i), qkv, M, self.qkvw, h)
                cache = self.kv_cache[i]
                self._kv_append(i, ly, qkv, M, Cc, shift, c0)
                if kv8:
                    sc = self.kv_scale[i]
                    H.kv8_dequant(cache, Smax * kvw, kvw, sc, Smax * 2 * hkv, 2 * hkv, kv_start, B, 2 * hkv, hd, c1, self.kv_stage, Smax * kvw, kvw)
                    kv = self.kv_stage
                else:
                    kv = cache
                H.attention_fwd(self._cache_attn_desc(qkv, kv, att, lse, B, Cc, c1, True, kv_start))
                H.gemm(att, ly["wo"], xm, M, h, aw, residual=x)
                H.rmsnorm_fwd(xm, ly["n2"], eps, hb, r)
                if blocked:
                    H.gemm(hb, ly["wgu_b"], gu, M, 2 * self.I, h, act=2, aux=act, ld_aux=self.I)
                else:
                    H.gemm(hb, ly["wgu"], gu, M, 2 * self.I, h)
                    H.swiglu_fwd(gu, act, M, self.I)
                H.gemm(act, ly["wd"], y, M, h, self.I, residual=xm)
                if layer_hook is not None:
                    layer_hook(i, y)
                x, y = y, x
        H.rmsnorm_fwd(x, self.norm, eps, hb, r)
        H.gemm(hb[Cc - 1:], self.head, last_logits, B, self.V, h, lda=Cc * h, ldc=self.Vp)     # row Cc - 1 of each sequence: A is a strided view
        return last_logits

    def _step_rows(self, tokens: torch.Tensor, cur: int, kv_start: torch.Tensor, layer_hook=None) -> torch.Tensor:
        """The KV-cached step, the one body of `decode_step` (w = 1) and `verify_step` (w = k + 1): `tokens` [B, w] (ids), row j of
        a sequence sits at cache slot cur + j (position = slot - left pad); returns logits [B * w, Vp] (batch-major), row j for
        slot cur + j + 1.  The row count M = B * w picks the buffer set, the projection kernel (MXFP4 decode weights: `gemm_w4` at
        every M; else M > 64 (`set_decode_rows`): `gemm_tall`, else M > 16: `gemm_wide`, else `gemm_w8` on FP8 decode weights, else `gemm`; the LoRA-merged q|k|v stays on `gemm`) and the RMSNorm fusion (`H.rms_fusable`); the
        rotated K | V go to slots [cur, cur + w) of the cache.  w picks the attention alone: w = 1 reads slots [kv_start, cur] without
        a mask, through the kv8 kernel under the FP8 cache, the split-KV kernel from H.DECODE_ATTN_MIN_KEYS keys on where the
        geometry allows, else the forward kernel; w > 1 reads slots [kv_start, cur + w) under the causal mask, the descriptor of
        `prefill`: through the forward kernel (bf16 cache), or with `set_speculative(attention="split")` through the split-KV verify
        kernels, on the bf16 cache by the w = 1 rule at `cur` where G w <= H.VERIFY_ATTN_MAX_ROWS, on the FP8 cache always.
        `layer_hook(l, x)` runs behind every layer on the step's rows [M, h]."""
        h, aw, eps = self.h, self.hq * self.hd, self.c.rms_norm_eps
        B, w = tokens.shape
        M = B * w
        bufs = self._step1 if w == 1 else self._spec_alloc(B, w - 1)
        x, xm, hb, qkv, att, act, r, lse, logits = (bufs[n] for n in ("x", "xm", "hb", "qkv", "att", "act", "r", "lse", "logits"))
        H.embed_gather(self.embed, None, tokens.reshape(-1).to(torch.int32), M, h, x)
        shift = (cur - kv_start).to(torch.int32).contiguous()                # position of the step's row j: cur + j - left pad
        fuse = H.rms_fusable(M, h)                      # RMSNorm folded into the projection that consumes it

        fp8 = self.decode_weights == "fp8"
        if fp8:
            self._fp8_decode_weights()

        mx = self.decode_weights == "mxfp4"
        if mx:
            self._mxfp4_decode_weights()

        def mm(xin, w_, w8, out, N, K, wide=M > 16, **kw):   # one projection on the bf16 weight, or on its e4m3 / MXFP4 copy (q, scale)
            if mx and w8 is not None:                   # every M up to H.DECODE_MAX_ROWS
                H.gemm_w4(xin, w8[0], w8[1], out, M, N, K, **kw)
            elif wide and M > H.DECODE_MAX_ROWS and w8 is None and tall_rows_to_gemm(M, 2 * N if kw.get("act") == 4 else N):
                if kw.get("act") == 4:                  # bf16 shapes the tile GEMM wins: the unfused gate|up + SwiGLU of `forward`
                    if bufs.get("gu") is None:          # [M, 2I], made by the first step of this set that takes the route
                        bufs["gu"] = self._b16(M, 2 * N)
                    H.gemm(xin, w_, bufs["gu"], M, 2 * N, K)
                    H.swiglu_fwd(bufs["gu"], out, M, N)
                else:
                    H.gemm(xin, w_, out, M, N, K, **kw)
            elif wide and M > H.DECODE_MAX_ROWS:        # M = 65..256 (`set_decode_rows`): still one weight pass
                H.gemm_tall(xin, w_ if w8 is None else w8[0], out, M, N, K, scale=None if w8 is None else w8[1], **kw)
            elif wide:                                  # M = 17..64: every weight byte once for all rows
                H.gemm_wide(xin, w_ if w8 is None else w8[0], out, M, N, K, scale=None if w8 is None else w8[1], **kw)
            elif w8 is not None:
                H.gemm_w8(xin, w8[0], w8[1], out, M, N, K, **kw)
            else:
                H.gemm(xin, w_, out, M, N, K, **kw)

        def proj(xin, nw, w_, w8, out, N, **kw):
            if fuse:
                mm(xin, w_, w8, out, N, h, a_rms_weight=nw, a_rms_eps=eps, **kw)
            else:
                H.rmsnorm_fwd(xin, nw, eps, hb, r)
                mm(hb, w_, w8, out, N, h, **kw)
        # long caches: split-KV kernel (K / V once per GQA group, a row's chunks on different CUs); a rule of the shape alone
        G = self.hq // self.hkv
        split_kv = self.hd == 128 and G <= 8 and cur + 1 >= H.DECODE_ATTN_MIN_KEYS
        if w > 1:                                       # the plain loop's rule at the step's first row, where the rows fit the MFMA's columns
            split_kv = split_kv and self.spec_attention == "split" and G * w <= H.VERIFY_ATTN_MAX_ROWS
        kv8 = self._gen_kind == "fp8"                   # FP8 cache: the kv8 kernels at every cur (the forward kernel cannot read bytes)
        ws = self.g_attn_ws if w == 1 else bufs.get("attn_ws")
        Smax = self._gen_shape[1]
        sc_bs, sc_rs = Smax * 2 * self.hkv, 2 * self.hkv
        one = dict(q_bs=self.qkvw, o_bs=aw) if w == 1 else {}
        for li, (ly, cache) in enumerate(zip(self.layers, self.kv_cache)):
            q8 = ly["q4"] if mx else ly["q8"] if fp8 else {}
            if self.lora is None:
                proj(x, ly["n1"], ly["wqkv"], q8.get("wqkv"), qkv, self.qkvw)
            else:                                                             # the merged weight stays on H.gemm at every M
                proj(x, ly["n1"], self._lora_merged(li), None, qkv, self.qkvw, wide=False)
            self._kv_append(li, ly, qkv, M, w, shift, cur)                   # rotate q,k + append K|V at slots [cur, cur + w)
            ad = self._cache_attn_desc(qkv, cache, att, lse, B, w, cur + w, w > 1, kv_start, **one)
            if kv8:
                (H.attention_decode_kv8 if w == 1 else H.attention_verify_kv8)(ad, self.kv_scale[li], self.kv_scale_v[li], sc_bs, sc_rs, ws)
            elif split_kv:
                (H.attention_decode if w == 1 else H.attention_verify)(ad, ws)
            else:
                H.attention_fwd(ad)
            mm(att, ly["wo"], q8.get("wo"), xm, h, aw, residual=x)
            proj(xm, ly["n2"], ly["wgu"], q8.get("wgu"), act, self.I, act=4)  # norm + gate|up projection + SwiGLU
            mm(act, ly["wd"], q8.get("wd"), x, h, self.I, residual=xm)
            if layer_hook is not None:                                        # ORCA deep injection on the new rows of every sequence
                layer_hook(li, x)
        proj(x, self.norm, self.head, self.head4 if mx else self.head8 if fp8 else None, logits, self.V, ldc=self.Vp)
        return logits

    def _verify_attn_rows(self, k: int) -> bool:
        """Whether the split-KV verify kernels take this geometry at k drafts: head_dim 128, G <= 8, G (k + 1) query rows per KV head
        within the score MFMA's 16 columns."""
        G = self.hq // self.hkv
        return self.hd == 128 and G <= 8 and G * (k + 1) <= H.VERIFY_ATTN_MAX_ROWS

    def decode_step(self, tokens: torch.Tensor, cur: int, kv_start: torch.Tensor, layer_hook=None) -> torch.Tensor:
        """One token per sequence: `tokens` [B] (ids) sit at cache slot `cur`; returns logits [B, Vp] for slot cur+1.  `_step_rows`
        at w = 1."""
        return self._step_rows(tokens.unsqueeze(1), cur, kv_start, layer_hook)

    # -- draft-and-verify greedy decoding (`set_speculative`): k + 1 rows per sequence through one pass over the weights ---------
    def _spec_alloc(self, B: int, k: int) -> dict:
        """The `_step_alloc` set of `verify_step` for B * (k + 1) rows, and the loop's integer state.  With
        `set_speculative(attention="split")` the set also holds `attn_ws`, the fp32 chunk partials of the split-KV verify attention
        for B * Hq * (k + 1) rows at the longest cache (None while that fits one chunk, or where the kernel does not take the
        geometry); it is made when first needed, so changing the attention alone keeps the set."""
        sp = self._spec
        if sp is not None and sp["key"] == (B, k):
            if self.spec_attention == "split" and sp.get("attn_ws_smax") != self._gen_shape[1]:
                ws = H.attention_verify_workspace_bytes(B, self.hq, k + 1, self._gen_shape[1], self.hd) if self._verify_attn_rows(k) else 0
                sp["attn_ws"] = None                                         # free the old one before the new one is made
                sp["attn_ws"], sp["attn_ws_smax"] = (torch.empty(ws // 4, dtype=F32, device=self.dev) if ws else None), self._gen_shape[1]
            return sp
        self._spec = sp = None                                               # free the old set before the new one is made
        dev, w = self.dev, k + 1

        def i64(*s):
            return torch.zeros(*s, dtype=torch.int64, device=dev)
        self._spec = sp = dict(key=(B, k), **self._step_alloc(B, w), pred=i64(B, w), inp=i64(B, w), draft=i64(B, k),
                               taken=torch.zeros(1, dtype=torch.int32, device=dev), taken_host=torch.zeros(1, dtype=torch.int32).pin_memory(),
                               event=torch.cuda.Event())
        return self._spec_alloc(B, k)

    def verify_step(self, tokens: torch.Tensor, cur: int, kv_start: torch.Tensor) -> torch.Tensor:
        """k + 1 tokens per sequence in one pass: `tokens` [B, k + 1] (ids >= 0; column 0 the last emitted token, columns 1..k the
        drafts), row j of a sequence sits at cache slot cur + j.  Returns logits [B * (k + 1), Vp] (batch-major): row j predicts
        slot cur + j + 1 GIVEN the chunk's tokens in front of it.  `_step_rows` at w = k + 1: `decode_step`'s body over
        M = B * (k + 1) rows (at most `row_limit`), with the causal attention over slots [kv_start, cur + k] (the forward
        kernel, or the split-KV verify kernels: `set_speculative(attention=...)`; the FP8 cache needs the latter).  Only slots in
        front of the next step's `cur` are ever trusted: the slots at or behind it hold drafts that were not accepted, and the next
        chunk rewrites them (its slot0 is the new `cur`, its width k + 1) before
        its attention, or any later one, reads them."""
        B, w = tokens.shape
        assert self._gen_shape[0] == B and B * w <= self.row_limit and cur + w <= self._gen_shape[1]
        assert self._gen_kind == "bf16" or (self.spec_attention == "split" and self._verify_attn_rows(w - 1))
        return self._step_rows(tokens, cur, kv_start)

    def _spec_reason(self, k, B, do_sample, use_pen, logprobs, forced_tokens, layer_hook, guided: bool = False,
                     constrained: bool = False) -> Optional[str]:
        """Why a call with speculation on runs the plain loop all the same; None when it does not.  A guided call (`guidance_scale`)
        always does.  The next four hold under scope "greedy" only (constrained: the call has an active `ConstraintPlan`); the FP8 KV
        cache is a reason unless `attention="split"` and the G (k + 1) query rows per KV head fit the verify kernel."""
        if guided:
            return "guidance_scale"
        if getattr(self, "spec_scope", "greedy") != "all":
            if do_sample:
                return "do_sample"
            if use_pen:
                return "repetition_penalty"
            if logprobs is not None:
                return "logprobs"
            if constrained:
                return "logit_constraints"
        if forced_tokens is not None:
            return "forced_tokens"
        if layer_hook is not None:
            return "layer_hook"
        if self.kv_cache_kind == "fp8":                                      # only the split-KV verify kernels read the byte cache
            if getattr(self, "spec_attention", "forward") != "split":
                return "fp8 kv cache"
            G = self.hq // self.hkv
            if G * (k + 1) > H.VERIFY_ATTN_MAX_ROWS:
                return f"fp8 kv cache: {G} x {k + 1} = {G * (k + 1)} query rows per KV head > {H.VERIFY_ATTN_MAX_ROWS}"
        if B * (k + 1) > self.row_limit:                                     # `set_decode_rows`; MXFP4 decode weights stay at the default
            return f"B * (k + 1) = {B * (k + 1)} rows > {self.row_limit}"
        return None

    @staticmethod
    def _trim_after_eos(out: torch.Tensor, eos: Optional[torch.Tensor], n_new: int) -> int:
        """n_new without the columns of `out` [B, >= n_new] behind the point where every sequence has produced an EOS."""
        if eos is None or n_new <= 1:
            return n_new
        hit = (out.unsqueeze(2) == eos.view(1, 1, -1)).any(dim=2)
        done_at = hit.int().argmax(dim=1)
        return min(n_new, int(torch.where(hit.any(dim=1), done_at + 1, torch.full_like(done_at, n_new)).max()))

    def _speculative_loop(self, logits, out, finished, eos, S: int, k: int, kv_start, pad_token_id: int, collect_logits: bool, draft_tokens, lookup_ids,
                          pick: Optional[dict] = None, pen_hist: Optional[torch.Tensor] = None, logprobs: Optional[int] = None,
                          constraints: Optional["ConstraintPlan"] = None):
        """The decode loop of `generate_greedy` with k drafts per step, on its `out` [B, T] / `finished` / `eos`.  Token 0 is the
        prompt pass's; then, with n tokens emitted and the last of them (not yet in the cache) due at slot cur = S + n - 1: draft ->
        `verify_step` on [last, drafts] -> the pick of all M rows -> `H.spec_accept`, which emits a >= 1 tokens for every row (the
        run all unfinished rows accept, the correction behind it included) and hands back a through a pinned int32: ONE host wait
        per verify step.
        The pick is the plain loop's for emitted position n + j (`pick`, scope "all"): argmax for plain greedy (pick None);
        `H.sample_rows` for the chain (repetition penalty, top_k, min_p, typical_p / epsilon / eta cut-offs; both do_sample modes) and `H.sample_top_p_rows` otherwise,
        at step0 = n.  Two histories are kept apart.  The penalty's is HF's `input_ids`, `pen_hist` [B, Pp + T]: the prompt ids of a
        text-only chat (left pads included), then the emitted tokens, pad for finished rows; `out` is its tail (a view), so the
        accept kernel's store into `out` is the store into it, and row j adds the chunk's j drafts in front of it.  The lookup
        history carries -1 at pads and audio slots and holds the spliced transcription; the accept kernel writes it as well.
        logprobs = n: one `H.topk_logprobs` launch over the M rows per verify step, in front of the host wait; row (b, j) scores the
        token it emits, -1 (0 / -1 / 0) on a row finished before the step or behind the first EOS of its run.
        constraints (an active `ConstraintPlan`; `pen_hist` is then set as well): one `H.logit_constraints` launch in front of
        every pick writes the banned scores into a [B (k + 1), Vp] scratch the pick reads, row (b, j) with the history `pen_hist[b,
        :Pp + n]` + the chunk's j drafts at emitted position n + j, as the plain loop bans there; `logprobs` and collect_logits
        keep reading the raw rows."""
        dev, w, (B, T) = self.dev, k + 1, out.shape
        sp = self._spec_alloc(B, k)
        pred, inp, draft, taken, taken_host, event = (sp[n] for n in ("pred", "inp", "draft", "taken", "taken_host", "event"))
        hist = row_start = None
        P = 0
        Pp = 0 if pen_hist is None else int(pen_hist.shape[1]) - T
        con_scores = None
        if constraints is not None:                                          # made once per shape; the kernel leaves the zero pad columns alone
            if getattr(self, "_con_scratch", None) is None or self._con_scratch.shape != (B * w, self.Vp):
                self._con_scratch = torch.zeros(B * w, self.Vp, dtype=BF16, device=dev)
            con_scores = self._con_scratch

        def first_pick(logits):                                              # the plain loop's launch at step 0
            if constraints is not None:
                constraints.apply(logits, self.Vp, con_scores, self.Vp, B, 1, self.V, pen_hist, Pp, step0=0)
                logits = con_scores
            if pick is None:
                H.argmax_bf16(logits, self.Vp, B, self.V, self.g_next)
            elif pick["chain"]:
                H.sample(logits, self.Vp, B, self.V, self.g_next, do_sample=pick["do_sample"], temperature=pick["temperature"], top_k=pick["top_k"],
                         top_p=pick["top_p"], min_p=pick["min_p"], repetition_penalty=pick["repetition_penalty"], hist=pen_hist, hist_len=Pp,
                         seed=pick["seed"], step=0, **pick["truncation"])
            else:
                H.sample_top_p(logits, self.Vp, B, self.V, pick["temperature"], pick["top_p"], pick["seed"], 0, self.g_next)

        def verify_pick(vl, n):                                              # row j: the plain loop's launch at step n + j
            if constraints is not None:
                constraints.apply(vl, self.Vp, con_scores, self.Vp, B, w, self.V, pen_hist, Pp + n, tail=inp, step0=n)
                vl = con_scores
            if pick is None:
                H.argmax_bf16(vl, self.Vp, B * w, self.V, pred)
            elif pick["chain"]:
                H.sample_rows(vl, self.Vp, B, w, self.V, pred, do_sample=pick["do_sample"], temperature=pick["temperature"], top_k=pick["top_k"],
                              top_p=pick["top_p"], min_p=pick["min_p"], repetition_penalty=pick["repetition_penalty"], hist=pen_hist,
                              hist_len=Pp + n, tail=inp, seed=pick["seed"], step0=n, **pick["truncation"])
            else:
                H.sample_top_p_rows(vl, self.Vp, B, w, self.V, pick["temperature"], pick["top_p"], pick["seed"], n, pred)
        if logprobs is not None:
            lp_tok = torch.zeros(B, T, dtype=F32, device=dev)
            lp_ids = torch.full((B, T, logprobs), -1, dtype=torch.int32, device=dev)
            lp_top = torch.zeros(B, T, logprobs, dtype=F32, device=dev)
            st_tok = torch.empty(B * w, dtype=F32, device=dev)               # one verify step's rows, contiguous for the kernel
            st_ids = torch.empty(B * w, logprobs, dtype=torch.int32, device=dev)
            st_top = torch.empty(B * w, logprobs, dtype=F32, device=dev)
        if draft_tokens is not None:                                         # the proposal for emitted position t, -1 = none
            props = torch.full((B, T + k), -1, dtype=torch.int64, device=dev)
            props[:, :T] = draft_tokens.to(dev, torch.int64)[:, :T]
        else:                                                                # lookup history: the prompt's ids (-1 = never matches), then the output
            P = 0 if lookup_ids is None else int(lookup_ids.shape[1])
            hist = torch.full((B, P + T), -1, dtype=torch.int64, device=dev)
            if P:
                hist[:, :P] = lookup_ids.to(dev, torch.int64)
            row_start = kv_start if P else torch.zeros(B, dtype=torch.int32, device=dev)
        steps_logits = [logits[:, :self.V].clone()] if collect_logits else None
        first_pick(logits)
        out[:, 0] = self.g_next
        if hist is not None:
            hist[:, P] = self.g_next
        if logprobs is not None:
            H.topk_logprobs(logits, self.Vp, self.g_next, B, self.V, logprobs, st_tok, st_ids, st_top)
            lp_tok[:, 0], lp_ids[:, 0], lp_top[:, 0] = st_tok[:B], st_ids[:B], st_top[:B]
        if eos is not None:
            finished |= (self.g_next.unsqueeze(1) == eos.unsqueeze(0)).any(dim=1)
        n, steps = 1, 0
        while n < T:                                                         # once every row is finished a = T - n: no early-exit check
            cur = S + n - 1
            if hist is None:
                draft.copy_(props[:, n:n + k])
            else:
                H.spec_ngram_draft(hist, P + n, row_start, k, SPEC_NGRAM_MAX, SPEC_NGRAM_MIN, draft)
            inp[:, 0] = self.g_next
            inp[:, 1:] = draft
            vl = self.verify_step(inp.clamp_min(0), cur, kv_start)          # a -1 draft is embedded as token 0 and can never be accepted
            verify_pick(vl, n)
            if logprobs is not None:                                         # `finished` is still the state in front of this step
                scored = torch.where(finished.unsqueeze(1), torch.full_like(pred, -1), pred)
                if eos is not None:                                          # the EOS itself is scored, the padding behind it is not
                    hit = (pred.unsqueeze(2) == eos.view(1, 1, -1)).any(dim=2).to(torch.int32)
                    scored = torch.where(hit.cumsum(dim=1) - hit > 0, torch.full_like(pred, -1), scored)
            H.spec_accept(pred, inp, k, finished, eos, pad_token_id, T - n, out, n, self.g_next, taken, hist=hist, hist_col=P + n)
            taken_host.copy_(taken, non_blocking=True)
            event.record()
            if logprobs is not None:                                         # an emitted token is the row's pick: columns [0, a) are read below
                H.topk_logprobs(vl, self.Vp, scored.contiguous(), B * w, self.V, logprobs, st_tok, st_ids, st_top)
            if collect_logits:
                rows = vl.view(B, w, self.Vp)[:, :, :self.V].transpose(0, 1).clone()      # [k + 1, B, V], before the wait
            event.synchronize()
            a = int(taken_host[0])
            if collect_logits:
                steps_logits.extend(rows[:min(a, w)])                        # a > k + 1 only once every row is finished: trimmed below
            if logprobs is not None:
                m = min(a, w)
                lp_tok[:, n:n + m] = st_tok.view(B, w)[:, :m]
                lp_ids[:, n:n + m] = st_ids.view(B, w, logprobs)[:, :m]
                lp_top[:, n:n + m] = st_top.view(B, w, logprobs)[:, :m]
            n += a
            steps += 1
        n_new = self._trim_after_eos(out, eos, n)
        self.spec_stats = dict(path="speculative", reason=None, verify_steps=steps, emitted=n_new, drafts_accepted=max(0, n_new - 1 - steps))
        out = out[:, :n_new]
        res = (out, torch.stack(steps_logits[:n_new])) if collect_logits else (out,)
        if logprobs is not None:
            res += (TokenLogprobs(token_logprobs=lp_tok[:, :n_new], top_ids=lp_ids[:, :n_new], top_logprobs=lp_top[:, :n_new]),)
        return res if len(res) > 1 else out

    def generate_greedy(self, x0_filler, B: int, S: int, kv_start: torch.Tensor, max_new_tokens: int, pad_token_id: int,
                        eos_token_ids=None, forced_tokens: Optional[torch.Tensor] = None, collect_logits: bool = False,
                        do_sample: bool = False, temperature: float = 1.0, top_p: float = 1.0, seed: int = 0, layer_hook=None,
                        after_prompt=None, top_k: Optional[int] = None, min_p: Optional[float] = None,
                        repetition_penalty: Optional[float] = None, prompt_ids: Optional[torch.Tensor] = None, chunk_hook=None,
                        logprobs: Optional[int] = None, speculate: Optional[int] = None, draft_tokens: Optional[torch.Tensor] = None,
                        lookup_ids: Optional[torch.Tensor] = None, guidance_scale: Optional[float] = None,
                        constraints: Optional["ConstraintPlan"] = None, typical_p: Optional[float] = None,
                        epsilon_cutoff: Optional[float] = None, eta_cutoff: Optional[float] = None):
        """Prompt pass + KV-cached decode (greedy, or temperature / top-p sampling with the library's counter RNG).  Returns new token ids [B, n_new] (int64; finished sequences are
        filled with pad_token_id, generation stops early once every sequence has produced an EOS), and, with
        collect_logits, the per-step logits [n_new, B, V] (bf16).  `forced_tokens` [B, T] teacher-forces the
        continuation (parity tests compare per-step logits with the oracle on the same prefix).  `layer_hook(l, x)` runs behind every
        decoder layer of the prompt pass ([B*S, h]; with `set_prefill_chunk` on the rows of one chunk, [B*Cc, h], `chunk_hook(i, Cc)` in
        front of chunk i) and of every decode step ([B, h]); `after_prompt()` between the two.
        top_k / min_p (sampling) and repetition_penalty (both modes) switch to HF's whole processor chain in one kernel
        (`desta_sample_bf16`); None = off.  The penalty's history is what HF's `input_ids` hold: `prompt_ids` [B, S] (text-only
        chats, left padding included) followed by the tokens emitted so far, pad_token_id for finished rows.
        logprobs = n (0..32): one more launch per step (`desta_topk_logprobs`) scores the step's token once it is fixed (forced /
        finished substitutions applied) and ranks the row's n most likely tokens; a `TokenLogprobs` is appended to the result.  The
        distribution is the MODEL'S OWN, log_softmax of the raw logits in front of the repetition penalty, the temperature and the
        top-k / top-p / min-p filters: HF's log_softmax(output_logits), not its processed output_scores.  The EOS token itself is
        scored; the padding behind it is not (0 / -1 / 0).  None: no launch, no allocation.
        speculate = k (1..7; None: the model's `set_speculative`, 0: off): draft-and-verify decoding, `_speculative_loop`; the
        plain loop below runs instead, and `spec_stats["reason"]` says why, under the conditions `set_speculative` lists (its
        scope "all" takes do_sample, repetition_penalty and logprobs off that list: the verify rows then go through the sampler
        this loop would launch, row j at step n + j, and the result is this loop's).  The
        drafts come from a lookup in `lookup_ids` [B, S] (the prompt's token ids, -1 at left pads and audio positions) followed by
        the emitted tokens, or from `draft_tokens` [B, max_new_tokens] (int64; the proposal for emitted position t, -1 = none).
        guidance_scale = g (None or 1: off, everything above as it stands): classifier-free guidance.  B = 2 Bc rows: rows [0, Bc) are
        the conditional prompts, row Bc + b the unconditional (negative) prompt of sequence b.  Prompt pass, cache and decode step
        run on all 2 Bc rows; per step one `H.cfg_scores` launch writes g * (lc - lu) + lu of the two halves' log-softmaxes into a
        [Bc, Vp] scratch and the pick above runs on that with rows = Bc (HF: the guidance processor is the first of the chain, so
        penalty, temperature and filters act on the guided scores); both rows of a sequence are fed its pick.  The result,
        `forced_tokens`, `prompt_ids` (the conditional prompts') and `logprobs` have Bc rows; EOS is judged per sequence.
        `logprobs` still reports the model's own distribution: the raw CONDITIONAL rows.  collect_logits returns the raw logits of
        all rows, [n_new, 2 Bc, V], conditional rows first: the values the guidance kernel read.  Speculation does not cover a
        guided call (`spec_stats["reason"] == "guidance_scale"`).
        constraints (a `ConstraintPlan`; None or an inactive one: off, no launch, no allocation): HF's banning processors,
        no_repeat_ngram_size / bad_words_ids / suppress_tokens / begin_suppress_tokens / min_new_tokens.  One
        `H.logit_constraints` launch per step sets the banned scores to -inf in front of the pick (and behind `H.cfg_scores`: in
        place on the guided scores); every other score keeps its bits, and the pickers never keep a -inf score.  The history the
        rules see is the penalty's above, kept with a plan even without a chain.  Without guidance the pass runs in place on the
        step's logits, or into a [Bc, Vp] scratch when `logprobs` or collect_logits read them: those keep reporting the raw model
        output.  A row with every token banned yields token 0.  Under `set_speculative(k, scope="all")` the verify rows go through
        the same pass (`_speculative_loop`); under scope "greedy" the plain loop runs (`spec_stats["reason"] == "logit_constraints"`).
        typical_p / epsilon_cutoff / eta_cutoff (None, 1.0 and 0.0 / 0.0: off; sampling only, ignored with do_sample=False as HF's
        warpers are): HF's TypicalLogitsWarper, EpsilonLogitsWarper and EtaLogitsWarper behind min-p, steps 7-9 of
        `desta_sample_truncated_rows_bf16`.  Any of them selects the chain kernel, which runs them in the same launch; guidance and
        constraints stay in front of it, `logprobs` and collect_logits keep reporting the raw distribution, and under
        `set_speculative(k, scope="all")` the verify rows take the same three values through the grouped call."""
        assert max_new_tokens >= 1
        check_guidance_arg(guidance_scale)
        guided = guidance_scale is not None and float(guidance_scale) != 1.0
        if guided and B % 2:
            raise ValueError(f"generate: guidance_scale needs an even number of rows (conditional rows, then one unconditional row each), got {B}")
        self.check_rows(B, guided)
        Bc = B // 2 if guided else B                                        # sequences: rows of the result and of every per-call state
        use_pen = repetition_penalty is not None and float(repetition_penalty) != 1.0
        trunc = truncation_kwargs(do_sample, typical_p, epsilon_cutoff, eta_cutoff)
        chain = use_pen or (do_sample and ((top_k is not None and int(top_k) != 0) or (min_p is not None and float(min_p) > 0.0) or bool(trunc)))
        check_speculative_arg(speculate)
        spec_k = (self.speculative if speculate is None else speculate) or 0
        con = constraints if constraints is not None and constraints.active else None
        spec_reason = self._spec_reason(spec_k, B, do_sample, use_pen, logprobs, forced_tokens, layer_hook, guided=guided,
                                        constrained=con is not None) if spec_k else "off"
        # a verify chunk writes up to k slots past the last accepted one: cache, cos / sin table and workspaces get k more slots
        Smax = S + max_new_tokens + (spec_k if spec_reason is None else 0)
        self._gen_alloc(B, Smax)
        dev = self.dev
        kv_start = kv_start.to(torch.int32).contiguous()
        neg_pad = (-kv_start).contiguous()                                   # prompt: position = index - left_pad
        logits = self._step1["logits"]                                       # the prompt's last row goes where the first pick reads
        if self._prompt_chunk(B) is not None:                                # lean prompt pass: chunks on rolling buffers, no save set
            self.prefill(x0_filler, B, S, kv_start, logits, layer_hook=layer_hook, chunk_hook=chunk_hook)
        else:
            self.forward(x0_filler, B, S, kv_start, None, False, pos_shift=neg_pad, cos_sin=self.gen_cos_sin, last_logits=logits,
                         kv_cache=self.kv_cache, layer_hook=layer_hook)
        if after_prompt is not None:
            after_prompt()
        out = torch.full((Bc, max_new_tokens), int(pad_token_id), dtype=torch.int64, device=dev)
        finished = torch.zeros(Bc, dtype=torch.bool, device=dev)
        eos = None if not eos_token_ids else torch.tensor(list(eos_token_ids), dtype=torch.int64, device=dev)
        P = 0
        if chain or con is not None:                                         # token history = [prompt ids,] emitted tokens: out is its tail
            P = 0 if prompt_ids is None else int(prompt_ids.shape[1])
            hist = torch.full((Bc, P + max_new_tokens), int(pad_token_id), dtype=torch.int64, device=dev)
            if P:
                hist[:, :P] = prompt_ids.to(dev, torch.int64)
            out = hist[:, P:]
        if spec_reason is None:
            pick = None
            if chain or do_sample:                                           # scope "all": the plain loop's sampler, one row per emitted position
                pick = dict(chain=chain, do_sample=do_sample, temperature=float(temperature), top_k=int(top_k or 0), top_p=float(top_p),
                            min_p=float(min_p or 0.0), repetition_penalty=float(repetition_penalty) if use_pen else 1.0, seed=seed,
                            truncation=trunc)
            return self._speculative_loop(logits, out, finished, eos, S, spec_k, kv_start, int(pad_token_id), collect_logits, draft_tokens, lookup_ids,
                                          pick=pick, pen_hist=hist if chain or con is not None else None, logprobs=logprobs, constraints=con)
        steps_logits = []
        if logprobs is not None:
            lp_tok = torch.zeros(Bc, max_new_tokens, dtype=F32, device=dev)
            lp_ids = torch.full((Bc, max_new_tokens, logprobs), -1, dtype=torch.int32, device=dev)
            lp_top = torch.zeros(Bc, max_new_tokens, logprobs, dtype=F32, device=dev)
            st_tok = torch.empty(Bc, dtype=F32, device=dev)                  # one step's rows, contiguous for the kernel
            st_ids = torch.empty(Bc, logprobs, dtype=torch.int32, device=dev)
            st_top = torch.empty(Bc, logprobs, dtype=F32, device=dev)
        n_new = 0
        g_next = self.g_next[:Bc]
        scores = logits                                                      # what the pick reads: the logits, or the guided scores
        if guided:                                                           # made once per shape; the kernel leaves the zero pad columns alone
            if getattr(self, "_cfg_scratch", None) is None or self._cfg_scratch.shape != (Bc, self.Vp):
                self._cfg_scratch = torch.zeros(Bc, self.Vp, dtype=BF16, device=dev)
            scores = self._cfg_scratch
        elif con is not None and (logprobs is not None or collect_logits):   # the raw logits are read again: the banned copy goes elsewhere
            if getattr(self, "_con_scratch", None) is None or self._con_scratch.shape != (Bc, self.Vp):
                self._con_scratch = torch.zeros(Bc, self.Vp, dtype=BF16, device=dev)
            scores = self._con_scratch
        for t in range(max_new_tokens):
            if collect_logits:
                steps_logits.append(logits[:, :self.V].clone())
            if guided:
                H.cfg_scores(logits[:Bc], logits[Bc:], self.Vp, Bc, self.V, float(guidance_scale), scores, self.Vp)
            if con is not None:                                              # guided: in place on the guided scores
                con.apply(scores if guided else logits, self.Vp, scores, self.Vp, Bc, 1, self.V, hist, P + t, step0=t)
            if chain:
                H.sample(scores, self.Vp, Bc, self.V, g_next, do_sample=do_sample, temperature=float(temperature),
                         top_k=int(top_k or 0), top_p=float(top_p), min_p=float(min_p or 0.0),
                         repetition_penalty=float(repetition_penalty) if use_pen else 1.0, hist=hist, hist_len=P + t, seed=seed, step=t,
                         **trunc)
            elif do_sample:
                H.sample_top_p(scores, self.Vp, Bc, self.V, float(temperature), float(top_p), seed, t, g_next)
            else:
                H.argmax_bf16(scores, self.Vp, Bc, self.V, g_next)
            nxt = g_next if forced_tokens is None else forced_tokens[:, t].to(dev, torch.int64)
            nxt = torch.where(finished, torch.full_like(nxt, int(pad_token_id)), nxt)
            out[:, t] = nxt
            if logprobs is not None:                                         # rows finished before this step carry -1: not read, 0 / -1 / 0
                H.topk_logprobs(logits, self.Vp, torch.where(finished, torch.full_like(nxt, -1), nxt), Bc, self.V, logprobs, st_tok, st_ids, st_top)
                lp_tok[:, t] = st_tok
                lp_ids[:, t] = st_ids
                lp_top[:, t] = st_top
            n_new = t + 1
            if eos is not None:
                finished |= (nxt.unsqueeze(1) == eos.unsqueeze(0)).any(dim=1)
                if (t & 7) == 7 and bool(finished.all()):                    # host sync only every 8 tokens
                    break
            if t + 1 == max_new_tokens:
                break
            logits = self.decode_step(torch.cat([nxt, nxt]) if guided else nxt, S + t, kv_start, layer_hook=layer_hook)
        n_new = self._trim_after_eos(out, eos, n_new)
        self.spec_stats = dict(path="plain", reason=spec_reason, verify_steps=0, emitted=n_new, drafts_accepted=0)
        out = out[:, :n_new]
        res = (out, torch.stack(steps_logits[:n_new])) if collect_logits else (out,)
        if logprobs is not None:
            res += (TokenLogprobs(token_logprobs=lp_tok[:, :n_new], top_ids=lp_ids[:, :n_new], top_logprobs=lp_top[:, :n_new]),)
        return res if len(res) > 1 else out

    def loss_and_grad(self, labels: torch.Tensor, write_grad: bool) -> torch.Tensor:
        """ForCausalLMLoss on the logits of the last forward; with write_grad the logits buffer becomes dlogits."""
        if getattr(self, "compact", None) is not None:
            idx, lab_c, Mc = self.compact
            if Mc == 0:
                self.loss.zero_()                                                            # ForCausalLMLoss of an all-ignored batch
                return self.loss
            H.causal_lm_loss(self.logits, self.Vp, lab_c, 1, Mc + 1, self.V, self.loss, write_grad=write_grad)
            return self.loss
        H.causal_lm_loss(self.logits, self.Vp, labels, self.B, self.S, self.V, self.loss, write_grad=write_grad)
        return self.loss

    def backward(self, first_needed_pos: int = 0, out_rows: Optional[Tuple[int, int]] = None, layer_hook_bwd=None) -> torch.Tensor:
        """dlogits (in self.logits) -> dL/d inputs_embeds [B*S, h] bf16.  In the position-major training layout only the rows of
        positions >= first_needed_pos (the first audio span of the batch) are propagated: the rows in front of it are frozen
        text embeddings whose gradient nothing consumes (under the causal mask they do not feed any needed row either).
        Two more dead-row cuts in that layout: (a) the last layer's gradient is zero in front of the first target position
        (`tail0`, set by forward), so its MLP / o_proj backward runs on the tail only; (b) `out_rows` = (first, last + 1) positions
        of the audio spans: the caller reads d inputs_embeds at those rows only, so layer 0's q|k|v input gradient and norm
        backward run on them alone (every other row of the returned buffer is then unspecified)."""
        c, h, M, S, B = self.c, self.h, self.M, self.S, self.B
        if self.lora is not None:
            first_needed_pos, out_rows = 0, None             # adapter gradients of the keys / values in front of the first audio span
        r0 = first_needed_pos * B if self.s_major else 0
        Mr = M - r0
        tl = max(self.tail0, r0) if self.s_major else r0        # last layer: rows [r0, tl) have zero gradient (forward skipped them)
        smb = B if self.s_major else 0
        dhb = self.hb
        if getattr(self, "compact", None) is not None and self.compact[2] == 0:
            self.dxa.zero_()                                                              # no target: every gradient is zero
            return self.dxa
        if getattr(self, "compact", None) is not None:
            idx, _, Mc = self.compact
            H.gemm(self.logits, self.headT, self.hbc, Mc, h, self.Vp, ldb=self.Vp)       # d(final norm out) of the target rows
            dhb[r0:].zero_()                                                              # the other rows have zero gradient
            H.scatter_rows(self.hbc, idx, Mc, h, dhb)
        else:
            H.gemm(self.logits, self.headT, dhb, M, h, self.Vp, ldb=self.Vp)
        dx, other = self.dxa, self.dxb
        if tl > r0:
            # forward skipped these rows of the last layer (stale activations): their gradients are exactly zero
            dx[r0:tl].zero_()
            other[r0:tl].zero_()
            self.datt[r0:tl].zero_()
        if M - tl > 0:
            H.rmsnorm_bwd(dhb[tl:], self.xs[self.L][tl:], self.norm, self.rf[tl:], dx[tl:])
        aw = self.hq * self.hd
        for i in reversed(range(self.L)):
            ly, s = self.layers[i], self.sv[i]
            if layer_hook_bwd is not None:                                                    # ORCA: back through the injection behind this layer (dx in place)
                layer_hook_bwd(i, dx)
            a0 = tl if i == self.L - 1 else r0                                                # first row with a non-zero d(layer output)
            Ma = M - a0
            if Ma > 0:
                if s.get("gu_blocked"):
                    # d(act) never reaches HBM: the epilogue of its GEMM forms d(gate|up) from the saved projection
                    H.gemm(dx[a0:], ly["wdT"], self.dgu[a0:], Ma, self.I, h, act=3, aux=s["gu"][a0:], ld_aux=2 * self.I, ldc=2 * self.I)
                    H.gemm(self.dgu[a0:], ly["wguT_b"], dhb[a0:], Ma, h, 2 * self.I)
                else:
                    if "wguT" not in ly:
                        ly["wguT"] = self._T(ly["wgu"])
                    H.gemm(dx[a0:], ly["wdT"], self.act[a0:], Ma, self.I, h)                  # d act
                    H.swiglu_bwd(s["gu"][a0:], self.act[a0:], self.dgu[a0:], Ma, self.I)
                    H.gemm(self.dgu[a0:], ly["wguT"], dhb[a0:], Ma, h, 2 * self.I)
                H.rmsnorm_bwd(dhb[a0:], s["xm"][a0:], ly["n2"], s["r2"][a0:], other[a0:], dres=dx[a0:])   # other := d x_mid
                H.gemm(other[a0:], ly["woT"], self.datt[a0:], Ma, aw, h)
            # attention backward runs on the whole grid (rows < r0 of datt stay zero; their dQ / the dK,dV of those keys are unused)
            fused = getattr(self, "_rope_fused", False)
            rcs = self.cos_sin_il if fused else None                 # fused: dQ / dK leave the attention backward already rotated back
            if self.s_major:
                H.attention_bwd(s["ad"], self.datt, self.dqkv, self.dqkv, self.dqkv, dq_off=0, dk_off=aw, dv_off=(self.hq + self.hkv) * self.hd,
                                do_rs=B * aw, dq_rs=B * self.qkvw, dk_rs=B * self.qkvw, dv_rs=B * self.qkvw,
                                do_bs=aw, dq_bs=self.qkvw, dk_bs=self.qkvw, dv_bs=self.qkvw, rope_cos_sin=rcs)
            else:
                H.attention_bwd(s["ad"], self.datt, self.dqkv, self.dqkv, self.dqkv, dq_off=0, dk_off=aw, dv_off=(self.hq + self.hkv) * self.hd,
                                rope_cos_sin=rcs)
            if not fused:
                H.rope(self.dqkv, self.qkvw, M, S, self.hq, self.hkv, self.hd, self.cos_sin, ly.get("qn"), ly.get("kn"), c.rms_norm_eps,
                       pre_norm=s.get("pre"), ld_pre=self.qkvw, backward=True, s_major_batch=smb)
            o0, o1 = r0, M
            if i == 0 and out_rows is not None and self.s_major and self.skip_dead_rows:
                o0, o1 = max(r0, out_rows[0] * B), min(M, out_rows[1] * B)                    # d inputs_embeds is read at the audio rows only
            H.gemm(self.dqkv[o0:], ly["wqkvT_il" if fused else "wqkvT"], dhb[o0:], o1 - o0, h, self.qkvw)
            if self.lora is not None:
                self._lora_bwd(i, ly, s, dhb, M)
            H.rmsnorm_bwd(dhb[o0:o1], self.xs[i][o0:o1], ly["n1"], s["r1"][o0:o1], dx[o0:o1], dres=other[o0:o1])   # dx := d x_in
        return dx


# =========================================================================================== the model
class DeSTA25AudioModel:
    """Drop-in for the reference's `DeSTA25AudioModel` on the qformer_1 path (hot path only)."""
    config_class = DeSTA25Config

    def __init__(self, config: DeSTA25Config, weights: Optional[Dict[str, torch.Tensor]] = None, device="cuda:0", **kwargs):
        if not torch.cuda.is_available():
            raise RuntimeError("DeSTA25AudioModel (MI355X hot path) needs a HIP device; there is no CPU fallback")
        self.config = config
        self.device = torch.device(device)
        self.audio_locator, self.placeholder_token = config.audio_locator, config.placeholder_token
        if weights is None:
            weights = self._load_base_weights(config)
        shapes = connector_param_shapes(config)
        shapes.update(lora_param_shapes(config))                       # use_lora: the decoder's q/k/v adapters are trainable too
        self.arena = ParamArena(list(shapes.items()), self.device)
        self.trainable_parameter_names = list(shapes.keys())
        with torch.cuda.device(self.device):
            self.encoder = WhisperEncoderHIP(config, weights, self.device)
            self.llm = CausalLMHIP(config, weights, self.device)
            self.connector = QformerConnectorHIP(config, self.arena, self.device)
            if config.use_lora:
                self.llm.attach_lora(self.arena, config.lora_r, config.lora_alpha, config.lora_dropout)
            self.orca = OrcaHIP(config, self.connector, self.device) if config.connector_mode == "orca_hybrid" else None
            # the LLM checkpoint's own generation defaults (read only; `hf_generation_kwargs` applies them on request)
            gp = os.path.join(str(config.llm_model_id), "generation_config.json")
            self.llm_generation_config = {}
            if os.path.isfile(gp):
                with open(gp) as f:
                    self.llm_generation_config = json.load(f)
            # Whisper's own decoder, when the checkpoint carries it: generate() then transcribes speech clips that arrive without text
            # itself (modeling_desta25.py:1580-1590) instead of asking for an injected `asr`
            self.asr_decoder = None
            if (DEC + "embed_tokens.weight") in weights:
                gc = config.extra.get("whisper_generation_config")
                if gc is None:
                    gp = os.path.join(config.encoder_model_id, "generation_config.json")
                    if os.path.isfile(gp):
                        with open(gp) as f:
                            gc = json.load(f)
                self.asr_decoder = WhisperDecoderHIP(config, weights, self.device, gc)
        # tokens one audio occupies in the text stream in front of its transcription (modeling_desta25.py:535, 540, 1570-1574)
        self.audio_tokens = config.orca_global_num_tokens if self.orca is not None else config.prompt_size
        self._init_connector(weights)
        e = config.encoder_config
        self.enc_all = None
        self._enc_bufs: List[Optional[torch.Tensor]] = [None, None]      # tapped states of the current batch / of the prefetched next one
        self._enc_cur = 0
        self.training = True
        self._weights_dirty = True
        self._fwd = None
        self._enc_pending: List[tuple] = []    # prefetched encoder outputs not consumed yet: (tensor, version, N, buffer, event)
        self.dropout_seed = 0                  # per-rank stream id of the Q-Former dropout RNG (trainer sets rank)
        self.compact_lm_head = True            # training: lm_head / CE / its backward on target rows only
        self._tr_stream = self._tr_idx = self._tr_lab = self._tr_count = self._tr_count_host = None
        self._fwd_count = 0
        self._slot_cache: Dict[tuple, tuple] = {}

    # -- weights -------------------------------------------------------------------------------
    @staticmethod
    def _load_base_weights(config) -> Dict[str, torch.Tensor]:
        """Base LLM + Whisper weights from LOCAL HF directories (safetensors only; nothing is executed)."""
        from safetensors import safe_open
        out: Dict[str, torch.Tensor] = {}
        # (Whisper: the encoder for the hot path and, for the ASR leg of generate(), the decoder of the same checkpoint)
        for path, prefix, keep in ((config.llm_model_id, LLM, None), (config.encoder_model_id, "perception.whisper.", ("model.encoder.", "model.decoder."))):
            files = sorted(f for f in os.listdir(path) if f.endswith(".safetensors")) if os.path.isdir(path) else []
            if not files:
                raise FileNotFoundError(f"no *.safetensors under '{path}' (local HF model directory required; no hub access)")
            for fn in files:
                with safe_open(os.path.join(path, fn), framework="pt") as f:
                    for k in f.keys():
                        if keep is None or k.startswith(keep):
                            out[prefix + k] = f.get_tensor(k)
        return out

    def _init_connector(self, weights):
        """Load connector tensors from `weights` when present, else the reference's init (H4):
        torch-default nn.Linear / LayerNorm init, randn prompts, zero mix weights."""
        g = torch.Generator().manual_seed(0)
        for name, shape in self.arena.shapes.items():
            if name in weights:
                self.arena.param(name).copy_(weights[name].to(self.device, F32).reshape(shape))
                continue
            if ".lora_B." in name:
                v = torch.zeros(*shape)                                # peft: B = 0, A = kaiming_uniform(a = sqrt 5) = U(+-1/sqrt(fan_in)), the `.weight` rule below
            elif "layer_prompts" in name or "global_queries" in name:
                v = torch.randn(*shape, generator=g)
            elif name.endswith("layer_weights"):
                v = torch.zeros(*shape)
            elif "LayerNorm" in name or "proj.0." in name.replace("gate_proj", "") or ".local_ln." in name or ".ln." in name:
                v = torch.ones(*shape) if name.endswith("weight") else torch.zeros(*shape)
            elif name.endswith("gate_proj.2.weight"):                   # ORCAGatedCrossAttention.__init__ (:382-383): gate starts at sigmoid(gate_init)
                v = torch.zeros(*shape)
            elif name.endswith("gate_proj.2.bias"):
                v = torch.full(shape, self.config.orca_gate_init)
            elif name.endswith("in_proj_weight"):                       # nn.MultiheadAttention: xavier_uniform_, zero biases
                v = (torch.rand(*shape, generator=g) * 2 - 1) * math.sqrt(6.0 / (shape[0] + shape[1]))
            elif name.endswith("in_proj_bias") or name.endswith("cross_attn.out_proj.bias"):
                v = torch.zeros(*shape)
            elif name.endswith(".weight"):
                v = (torch.rand(*shape, generator=g) * 2 - 1) / math.sqrt(int(math.prod(shape[1:])))
            else:
                fan_in = int(math.prod(self.arena.shapes[name[:-4] + "weight"][1:]))
                v = (torch.rand(*shape, generator=g) * 2 - 1) / math.sqrt(fan_in)
            self.arena.param(name).copy_(v.to(self.device))

    def named_parameters(self):
        for n in self.trainable_parameter_names:
            yield n, self.arena.param(n)

    def state_dict(self):
        """Only the trainable parameters, like the reference (modeling_desta25.py:1284-1292)."""
        return OrderedDict((n, self.arena.param(n).detach().clone()) for n in sorted(self.trainable_parameter_names))

    def load_state_dict(self, state_dict, strict=True, assign=False):
        sd = {k.replace("ocar_cross_attns", "orca_cross_attns"): v for k, v in state_dict.items()}
        glw = sd.get(CON + "global_layer_weights")
        if glw is not None and self.orca is not None and int(glw.shape[1]) != len(self.config.target_layer_ids):
            # layer-count mismatch (:1311-1345): re-tap the encoder and rebuild the trainable half (arena, connector, injection) before
            # copying — an optimizer made for the old arena must be re-created, exactly as with the reference's new connector module
            self.config.align_orca_layers(int(glw.shape[1]))
            logging.warning("checkpoint taps %d encoder layers: rebuilding the ORCA connector (orca_use_all_layers=%s)", glw.shape[1], self.config.orca_use_all_layers)
            shapes = connector_param_shapes(self.config)
            shapes.update(lora_param_shapes(self.config))
            self.arena = ParamArena(list(shapes.items()), self.device)
            self.trainable_parameter_names = list(shapes.keys())
            with torch.cuda.device(self.device):
                self.connector = QformerConnectorHIP(self.config, self.arena, self.device)
                if self.config.use_lora:
                    self.llm.attach_lora(self.arena, self.config.lora_r, self.config.lora_alpha, self.config.lora_dropout)
                self.orca = OrcaHIP(self.config, self.connector, self.device)
            self._init_connector({})
            self.drop_prefetched()
            self.encoder.B = 0                                                 # the tap buffer changes its leading dimension
            self.enc_all, self._enc_bufs = None, [None, None]
        missing = [n for n in self.trainable_parameter_names if n not in sd]
        unexpected = [k for k in sd if k not in self.arena.shapes]
        if strict and (missing or unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict: missing {missing[:5]} unexpected {unexpected[:5]}")
        for n in self.trainable_parameter_names:
            if n in sd:
                self.arena.param(n).copy_(sd[n].to(self.device, F32).reshape(self.arena.shapes[n]))
        self._weights_dirty = True
        return missing, unexpected

    def save_pretrained(self, path: str, state_dict=None, **kwargs):
        from safetensors.torch import save_file
        os.makedirs(path, exist_ok=True)
        self.config.save_pretrained(path)
        sd = state_dict if state_dict is not None else self.state_dict()
        save_file({k: v.detach().cpu().contiguous() for k, v in sd.items()}, os.path.join(path, "model.safetensors"))

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, *args, **kwargs):
        """Config + base models from local dirs, then trainable-only model.safetensors (strict=False)."""
        from safetensors.torch import load_file
        config = cls.config_class.from_pretrained(pretrained_model_name_or_path)
        if not os.path.isdir(pretrained_model_name_or_path):
            raise FileNotFoundError(f"'{pretrained_model_name_or_path}' is not a local directory (no hub access)")
        sd = load_file(os.path.join(pretrained_model_name_or_path, "model.safetensors"))
        glw = sd.get(CON + "global_layer_weights")
        if glw is not None and config.align_orca_layers(int(glw.shape[1])):     # before anything is built (the reference rebuilds its connector)
            logging.warning("checkpoint taps %d encoder layers: orca_use_all_layers=%s, target_layer_ids=%s", glw.shape[1], config.orca_use_all_layers,
                            config.target_layer_ids if len(config.target_layer_ids) <= 8 else f"0..{config.target_layer_ids[-1]}")
        model = cls(config, **{k: v for k, v in kwargs.items() if k in ("weights", "device")})
        model.load_state_dict(sd, strict=False)
        return model

    def train(self, mode=True):
        self.training = mode
        return self

    def set_decode_weights(self, kind: str) -> None:
        """Weights the LLM's KV-cached decode steps stream: "bf16" (default), "fp8" (weight-only OCP e4m3, per-row power-of-two
        scales) or "mxfp4" (weight-only OCP MXFP4: e2m1 nibbles, one e8m0 scale per 32 elements; `CausalLMHIP.set_decode_weights`).
        `generate`, `_generate_step` and the trainer's evaluate use whatever is set."""
        kinds = CausalLMHIP.DECODE_WEIGHT_KINDS + CausalLMHIP.DECODE_WEIGHT_KINDS_MX
        if kind not in kinds:
            raise ValueError(f"decode_weights must be one of {kinds}, got {kind!r}")
        self.llm.set_decode_weights(kind)

    def set_kv_cache(self, kind: str) -> None:
        """What the LLM's KV cache holds during `generate` / `_generate_step` / the trainer's evaluate: "bf16" (default) or "fp8"
        (OCP e4m3 bytes + per-head power-of-two scales; `CausalLMHIP.set_kv_cache`).  ORCA's audio K|V and Whisper's ASR decoder
        keep their own bf16 caches."""
        if kind not in CausalLMHIP.KV_CACHE_KINDS:
            raise ValueError(f"kv_cache must be one of {CausalLMHIP.KV_CACHE_KINDS}, got {kind!r}")
        self.llm.set_kv_cache(kind)

    def set_prefill_chunk(self, n: Optional[int]) -> None:
        """Prompt pass of `generate` / `_generate_step` / the trainer's evaluate: None (default) = the training forward with its
        per-layer save set; an int >= 16 = the lean pass in chunks of n positions, whose memory outside the KV cache follows n
        instead of the prompt length and the layer count (`CausalLMHIP.set_prefill_chunk`).  `score` / `score_batch` need every
        position's logits and Whisper's ASR decoder has its own loop: both are unaffected."""
        check_prefill_chunk(n)
        self.llm.set_prefill_chunk(n)

    def set_decode_rows(self, n: Optional[int]) -> None:
        """Row ceiling of a KV-cached step of `generate` / `_generate_step` / the trainer's evaluate: None or 64 (default), or an
        int in 65..256 (`CausalLMHIP.set_decode_rows`): that many sequences per call, half of it under `guidance_scale`,
        B (k + 1) <= n under `set_speculative(k)`.  bf16 and FP8 decode weights; MXFP4 stays at 64 rows.  Above 64 audios the
        encoder and the connector run in slices, above 64 sequences the prompt pass is the lean chunked one.  Anything else raises
        ValueError and leaves the setting as it was."""
        check_decode_rows_arg(n)
        self.llm.set_decode_rows(n)

    def _perceive_sliced(self, feats: torch.Tensor, N: int) -> torch.Tensor:
        """Encoder + connector of N > PERCEPTION_SLICE audios in equal slices of at most PERCEPTION_SLICE, so that their scratch
        buffers are sized by a slice: self.enc_all [taps, N*T, d] and the returned audio features [N*K, h] hold, audio by audio,
        the rows one call over all N would have written."""
        self.drop_prefetched()                                               # the encoder's scratch is shared with pending prefetches
        e, con = self.config.encoder_config, self.connector
        T, nt = e.max_source_positions, len(self.config.target_layer_ids)
        self.enc_all = self._enc_buf(self._enc_cur, N)
        af = torch.empty(N * con.K, con.h, dtype=BF16, device=self.device)
        step = -(-N // -(-N // PERCEPTION_SLICE))
        part = torch.empty(nt, step * T, e.d_model, dtype=BF16, device=self.device)
        for a0 in range(0, N, step):
            n = min(step, N - a0)
            enc = part if n == step else torch.empty(nt, n * T, e.d_model, dtype=BF16, device=self.device)
            self.encoder.forward(feats[a0:a0 + n].to(self.device, F32).contiguous(), enc)
            self.enc_all[:, a0 * T:(a0 + n) * T].copy_(enc)
            af[a0 * con.K:(a0 + n) * con.K].copy_(con.forward(enc, n))
        return af

    def set_speculative(self, k: Optional[int], scope: str = "greedy", attention: str = "forward") -> None:
        """Decoding of `generate` / `_generate_step` / the trainer's evaluate: None or 0 (default) = one token per step; an
        int k in 1..7 = k draft tokens per step from a lookup in the row's own prompt (the spliced transcription included) and
        output, verified by one pass over the weights (`CausalLMHIP.set_speculative`, which lists what runs the plain loop
        instead).  scope = "greedy" (default): plain greedy calls only; scope = "all": sampled calls (the default of `generate`),
        a repetition penalty and `logprobs` speculate too and return the plain loop's tokens.  attention = "split": a verify step
        attends through the split-KV verify kernels, from H.DECODE_ATTN_MIN_KEYS keys on with the bf16 cache and at every length
        with the FP8 KV cache, which speculates only under this setting.  A bad k, scope or attention raises ValueError
        and leaves the setting as it was.  `model.llm.spec_stats` reports the path taken and the acceptance of the last call."""
        check_speculative_arg(k)
        check_speculative_scope(scope)
        check_speculative_attention(attention)
        self.llm.set_speculative(k, scope, attention)

    def eval(self):
        return self.train(False)

    def mark_weights_updated(self):
        self._weights_dirty = True

    def refresh_weights(self):
        """bf16 operand copies of every trainable tensor from the fp32 arena, on the current stream (the trainer calls this right
        behind the optimizer step; a forward does it itself when `mark_weights_updated` / `load_state_dict` flagged a change)."""
        self.connector.refresh_weights()
        if self.orca is not None:
            self.orca.refresh_weights()
        if self.llm.lora is not None:
            self.llm.lora["dirty"] = True
            self.llm.refresh_lora()

    # -- forward / backward ----------------------------------------------------------------------
    def _audio_slots(self, starts, B: int, S: int, s_major: bool):
        """Flat row indices of the audio slots of inputs_embeds ([N_audio * K] int64, device) and the source-map values that
        mark them (-(audio_row + 1), int32), cached per (starts, B, S, layout) signature: batches of one run share a handful of
        signatures, so neither forward nor backward rebuilds and re-uploads index tensors every step."""
        K = self.audio_tokens
        key = (tuple(starts), B, S, bool(s_major))
        hit = self._slot_cache.get(key)
        if hit is None:
            ar = torch.arange(K, dtype=torch.int64)
            pos = torch.cat([((s + ar) * B + r) if s_major else (r * S + s + ar) for r, s in starts])
            val = -(torch.arange(len(starts) * K, dtype=torch.int32) + 1)
            if len(self._slot_cache) >= 64:
                self._slot_cache.clear()
            hit = self._slot_cache[key] = (pos.to(self.device), val.to(self.device), pos.to(self.device, torch.int32))
        return hit

    def _src_rows(self, input_ids, batch_transcription_ids, batch_start_positions, audio_lengths, audio_index=None):
        """int32 map [B*S]: >=0 token row of the embedding table, <0 -(audio_row+1).  audio_index[a] (optional): the audio whose
        connector rows span a reads, when several spans share one encoded audio (`score`); default: span a reads audio a."""
        B, S = input_ids.shape
        K = self.audio_tokens
        src = input_ids.to(torch.int32).clone()
        starts = [(int(r), int(s)) for r, s in batch_start_positions]
        for a, (row, start) in enumerate(starts):
            assert start + K + batch_transcription_ids[a].numel() <= S, "audio span exceeds the sequence"
        if starts:
            pos, val, _ = self._audio_slots(starts, B, S, False)
            if audio_index is not None:
                val = -(torch.tensor(audio_index, dtype=torch.int32).view(-1, 1) * K + torch.arange(K, dtype=torch.int32) + 1).view(-1).to(src.device)
            src.view(-1).index_copy_(0, pos, val)                             # one launch for every audio span of the batch
        for a, (row, start) in enumerate(starts):
            tr = batch_transcription_ids[a].reshape(-1)
            if tr.numel():                                                    # (empty in training, hazard H9)
                src[row, start + K:start + K + tr.numel()] = tr.to(src.device, torch.int32)
        return src.reshape(-1).contiguous()

    def _h2d(self, t: torch.Tensor) -> torch.Tensor:
        """Host tensor of a collated batch -> device WITHOUT synchronising the stream: from pageable memory torch's copy is
        staged and waits for the stream to drain, which throws away the host's run-ahead over the ≈1900 queued launches of a step
        (measured with `bench.py --data wav`: +3.6 ms per step); from pinned memory (the DataLoader's `pin_memory`, or pinned here)
        it is an asynchronous copy on the current stream."""
        if t.device == self.device:
            return t
        if t.device.type == "cpu" and not t.is_pinned() and t.numel() > 0:
            t = t.pin_memory()
        return t.to(self.device, non_blocking=True)

    def forward(self, input_ids, attention_mask, batch_features, batch_transcription_ids, batch_start_positions,
                labels=None, **kwargs):
        cfg, dev = self.config, self.device
        B, S = input_ids.shape
        K = cfg.prompt_size
        input_ids = self._h2d(input_ids)
        attention_mask = self._h2d(attention_mask)
        if labels is not None:
            labels = self._h2d(labels)
        N_audio = len(batch_start_positions)
        # score(): audio_index[a] = row of batch_features that span a splices in (every answer option reads the one encoded audio)
        audio_index = kwargs.get("audio_index")
        N_enc = N_audio if audio_index is None or N_audio == 0 else int(batch_features.shape[0])
        with torch.cuda.device(dev):
            if self._weights_dirty:
                self.refresh_weights()
                self._weights_dirty = False
            af = None
            seed_base = _splitmix64(((self.dropout_seed & 0xFFFFFFFF) << 32) | (self._fwd_count & 0xFFFFFFFF))   # (rank stream, forward)
            if self.llm.lora is not None:
                self.llm.lora["seed_base"] = seed_base
            if N_audio > 0 or self.llm.lora is not None:
                self._fwd_count += 1
            if N_audio > 0:
                assert len(batch_start_positions) == len(batch_transcription_ids) == (batch_features.shape[0] if audio_index is None else len(audio_index)), \
                    "batch_start_positions, batch_transcription_ids, audio_features, speech_feature_lengths must have the same length."
                self._encode(batch_features, N_enc)
                self.connector.p_drop = cfg.qformer_dropout if self.training else 0.0
                self.connector.seed_base = seed_base
                af = self.connector.forward(self.enc_all, N_enc)
                if self.orca is not None and audio_index is not None:
                    # ORCA pairs audio row b with text row b: repeat the encoded audios' global tokens per span (the encoder ran once)
                    af = af.view(N_enc, -1, af.shape[-1])[torch.as_tensor(audio_index, device=dev)].reshape(-1, af.shape[-1]).contiguous()
                src = self._src_rows(input_ids, [self._h2d(t) for t in batch_transcription_ids], batch_start_positions, None,
                                     audio_index=None if self.orca is not None else audio_index)
            else:
                src = input_ids.to(torch.int32).reshape(-1).contiguous()
            kv_start = (attention_mask == 0).sum(dim=1).to(torch.int32).contiguous()
            h = cfg.llm_config.hidden_size
            # score_batch(): eval forward with the lm_head on the target rows only (batch-major grid; the logits stay logits)
            compact_eval = bool(kwargs.get("compact_targets", False)) and labels is not None and not self.training
            if self.orca is not None:
                return self._forward_orca(input_ids, attention_mask, batch_transcription_ids, batch_start_positions, labels, af, src, kv_start, N_audio,
                                          keep_logits=bool(kwargs.get("keep_logits", False)),
                                          target_rows=self._target_rows(labels, B, S) if compact_eval else None, audio_index=audio_index)

            def fill(buf):
                H.embed_gather(self.llm.embed, af, src, B * S, h, buf)
            target_rows = None
            s_major = False
            if (labels is not None and self.training and N_audio > 0 and not kwargs.get("keep_logits", False)
                    and self.compact_lm_head):
                # training fast path: position-major token grid (row = s * B + b) + lm_head on the target rows only
                s_major = True
                src = src.view(B, S).t().contiguous().view(-1)
                target_rows = self._target_rows(labels, B, S, s_major=True)
            elif compact_eval:
                target_rows = self._target_rows(labels, B, S)
            logits = self.llm.forward(fill, B, S, kv_start, labels, self.training, target_rows=target_rows, s_major=s_major)
            V = cfg.llm_config.vocab_size
            out_logits = None if compact_eval else logits.view(B, S, self.llm.Vp)[:, :, :V]
            loss = None
            if labels is not None:
                labels = labels.to(dev).contiguous()
                need_grad = self.training and (N_audio > 0 or self.llm.lora is not None)
                if need_grad:
                    # dlogits overwrite the logits buffer: hand the caller a copy only if asked to keep them
                    if kwargs.get("keep_logits", False):
                        out_logits = out_logits.clone()
                    else:
                        out_logits = None
                # clone: the kernel writes into a persistent 1-element buffer that the next step overwrites
                loss = self.llm.loss_and_grad(labels, write_grad=need_grad).clone().view(())
            # audio rows of inputs_embeds, for the backward gather
            self._fwd = dict(B=B, S=S, N_audio=N_audio, starts=[(int(r), int(s)) for r, s in batch_start_positions],
                             has_grad=labels is not None and self.training and (N_audio > 0 or self.llm.lora is not None), s_major=s_major)
        return _Out(loss, out_logits)

    def _forward_orca(self, input_ids, attention_mask, batch_transcription_ids, batch_start_positions, labels, af, src, kv_start, N_audio, keep_logits=False,
                      target_rows=None, audio_index=None):
        """The ORCA branch of the reference's forward (modeling_desta25.py:775-841): global tokens spliced at the audio
        positions, the local tokens injected behind every decoder layer through the gated cross-attention, LM loss + `orca_losses`
        (the trainer adds them up, desta_trainer.py:56-92).  Batch-major token grid; in training mode the activations the backward needs
        are kept (`OrcaHIP.sv`) and `backward()` returns the gradients of that total loss.  One audio per text row, in row
        order: the reference's cross-attention pairs audio row b with text row b (`query=hidden_states, key=audio_local`, :447-453)."""
        cfg, dev, orca = self.config, self.device, self.orca
        B, S = input_ids.shape
        hdim, V = cfg.llm_config.hidden_size, cfg.llm_config.vocab_size
        local16, spans = None, None
        need_grad = bool(self.training and labels is not None and N_audio > 0)
        if N_audio > 0:
            rows = [int(r) for r, _ in batch_start_positions]
            assert N_audio == B and rows == list(range(B)), "orca_hybrid: one audio per text row, in row order"
            if audio_index is None:
                local16 = orca.local_forward(self.enc_all, N_audio)
            else:                                                                # score(): local tokens of each encoded audio, repeated per text row
                n_enc = int(self.enc_all.shape[1]) // cfg.encoder_config.max_source_positions
                local16 = orca.local_forward(self.enc_all, n_enc)
                if local16 is not None:
                    local16 = local16.view(n_enc, -1, hdim)[torch.as_tensor(audio_index, device=dev)].reshape(-1, hdim).contiguous()
            Kg = cfg.orca_global_num_tokens
            spans = [(int(r), int(s) + Kg, int(s) + Kg + int(t.numel())) for (r, s), t in zip(batch_start_positions, batch_transcription_ids)]
            orca.begin(af, local16, B, S, spans, self.training, save=need_grad)
            hook = orca.inject
        else:
            orca.audio, orca.aligns = None, []
            hook = None

        def fill(buf):
            H.embed_gather(self.llm.embed, af, src, B * S, hdim, buf)
        logits = self.llm.forward(fill, B, S, kv_start, labels, need_grad, layer_hook=hook, target_rows=target_rows)
        out_logits = None if target_rows is not None else logits.view(B, S, self.llm.Vp)[:, :, :V]
        loss = None
        if labels is not None:
            if need_grad and out_logits is not None:                         # dlogits overwrite the logits buffer (as on the qformer_1 path)
                out_logits = out_logits.clone() if keep_logits else None
            loss = self.llm.loss_and_grad(labels.to(dev).contiguous(), write_grad=need_grad).clone().view(())
        out = _Out(loss, out_logits)
        out.orca_losses = orca.losses(af, local16, B) if N_audio > 0 else OrderedDict()
        out.audio_global = af.view(B, cfg.orca_global_num_tokens, hdim) if N_audio > 0 else None
        out.audio_local = local16.view(B, -1, hdim) if local16 is not None else None
        self._fwd = dict(orca=True, has_grad=need_grad, B=B, S=S, N_audio=N_audio, starts=[(int(r), int(s)) for r, s in batch_start_positions], s_major=False)
        return out

    __call__ = forward

    @torch.no_grad()
    def _generate_step(self, inputs, pad_token_id, temperature=0.7, top_p=0.9, max_new_tokens=512, do_sample=True,
                       eos_token_id=None, forced_tokens=None, collect_logits=False, seed=0, top_k=None, min_p=None,
                       repetition_penalty=None, prompt_in_history=False, logprobs=None, draft_tokens=None, guidance_scale=None,
                       no_repeat_ngram_size=None, bad_words_ids=None, suppress_tokens=None, begin_suppress_tokens=None, min_new_tokens=None,
                       typical_p=None, epsilon_cutoff=None, eta_cutoff=None):
        """Reference `_generate_step` (modeling_desta25.py:1358-1431): audio features spliced into the prompt
        embeddings, then `llm_model.generate(inputs_embeds=…)` — here the KV-cached decoder on the HIP path.
        Returns ONLY the new tokens, as HF does for inputs_embeds prompts.  do_sample=False: greedy (temperature / top_p
        ignored, as the reference nulls them).  do_sample=True: temperature -> top-p -> one multinomial draw per step
        with the library's counter RNG (`seed`; same distribution as HF, not torch's random stream).
        top_k, min_p (sampling only) and repetition_penalty (both modes) add HF's TopK / MinP warpers and its
        RepetitionPenaltyLogitsProcessor; None = off.  HF's history for the penalty is `input_ids`: empty for an
        inputs_embeds prompt (only the generated tokens count, TF:generation/utils.py:1176-1181), the prompt ids for a text
        prompt passed as input_ids (`prompt_in_history=True`, the text-only leg of `generate`).
        logprobs = n: a `TokenLogprobs` becomes the last element of the result, (ids, lp) or (ids, logits, lp): every emitted
        token's log-probability and the n most likely tokens of its step under the model's own distribution, log_softmax of the
        raw logits (HF's output_logits, not the processed output_scores; see `CausalLMHIP.generate_greedy`).
        With `set_speculative(k)` greedy calls decode by draft and verify, and with `set_speculative(k, scope="all")` sampled,
        penalised and `logprobs` calls do too, with the plain loop's tokens and `TokenLogprobs`.
        The drafts are looked up in the row's prompt ids (the
        spliced transcription included, audio slots and pads never match) and its output, or taken from `draft_tokens`
        [B, max_new_tokens] (the proposal for emitted position t, -1 = none: tests and benchmarks).
        guidance_scale = g (None or 1: off): classifier-free guidance, HF's `guidance_scale` with a negative prompt.  `inputs` hold
        2 Bc rows, the Bc conditional prompts and then the unconditional prompt of each (audio spans may lie in any of them); the
        result and `forced_tokens` have Bc rows (`CausalLMHIP.generate_greedy`).  Not with ORCA deep injection.
        no_repeat_ngram_size / bad_words_ids / suppress_tokens / begin_suppress_tokens / min_new_tokens: HF's banning processors of
        the same names (NoRepeatNGram, NoBadWords, SuppressTokens, SuppressTokensAtBegin, MinNewTokensLength); None = off.  They see
        the penalty's history (empty for an inputs_embeds prompt, the prompt ids with `prompt_in_history`), `[eos]` bad words are
        dropped, min_new_tokens bans every EOS id for the first m emitted tokens, and begin_suppress_tokens act on the first one.
        One launch per step sets the banned scores to -inf in front of the pick and behind the guidance
        (`desta_logit_constraints_bf16`); `logprobs` and collect_logits keep the raw model output.  If every token of a step is
        banned the step yields token 0.
        typical_p / epsilon_cutoff / eta_cutoff: HF's TypicalLogitsWarper, EpsilonLogitsWarper and EtaLogitsWarper behind min-p, in
        the chain kernel's launch (`desta_sample_truncated_rows_bf16`); None, 1.0 and 0.0 / 0.0 = off, and with do_sample=False they
        are accepted and ignored, as HF's warpers are."""
        check_sampling_args(top_k, min_p, repetition_penalty)
        check_truncation_args(typical_p, epsilon_cutoff, eta_cutoff)
        check_logprobs_arg(logprobs)
        check_guidance_arg(guidance_scale)
        check_constraint_args(no_repeat_ngram_size, bad_words_ids, suppress_tokens, begin_suppress_tokens, min_new_tokens,
                              vocab=getattr(getattr(self, "llm", None), "V", None))
        constrained = any(v is not None for v in (no_repeat_ngram_size, bad_words_ids, suppress_tokens, begin_suppress_tokens, min_new_tokens))
        guided = guidance_scale is not None and float(guidance_scale) != 1.0
        if guided and self.orca is not None:
            raise NotImplementedError("guidance_scale with ORCA deep injection (orca_hybrid): the injection hook takes one audio per row, "
                                      "the unconditional rows of a guided batch have none")
        cfg, dev = self.config, self.device
        input_ids = inputs["context_input_ids"].to(dev)                      # only the context (prompt) part of the batch
        attention_mask = inputs["context_attention_mask"].to(dev)
        B, S = input_ids.shape
        if guided and B % 2:
            raise ValueError(f"guidance_scale: inputs hold the conditional rows and then one unconditional row each, got {B} rows")
        self.llm.check_rows(B, guided)                                       # before the encoder and the prompt pass run
        starts = inputs["context_batch_start_positions"]
        N_audio = len(starts)
        was_training = self.training
        self.training = False                                                # no Q-Former dropout while generating
        try:
            with torch.cuda.device(dev):
                if self._weights_dirty:
                    self.refresh_weights()
                    self._weights_dirty = False
                af = None
                if N_audio > 0:
                    feats = inputs["batch_features"]
                    trs = [t.to(dev) for t in inputs["batch_transcription_ids"]]
                    assert len(starts) == len(trs) == feats.shape[0]
                    self.connector.p_drop = 0.0
                    if N_audio > PERCEPTION_SLICE:                           # more audios than a default step has rows: buffers sized by a slice
                        af = self._perceive_sliced(feats, N_audio)
                    else:
                        self._encode(feats, N_audio)
                        af = self.connector.forward(self.enc_all, N_audio)
                    src = self._src_rows(input_ids, trs, starts, None)
                else:
                    src = input_ids.to(torch.int32).reshape(-1).contiguous()
                kv_start = (attention_mask == 0).sum(dim=1).to(torch.int32).contiguous()
                h = cfg.llm_config.hidden_size

                def fill(buf):
                    H.embed_gather(self.llm.embed, af, src, B * S, h, buf)
                hook = after = chunk = None
                if self.orca is not None and N_audio > 0:
                    # ORCA branch (modeling_desta25.py:1375-1408): global tokens spliced above; the audio tokens reach every decoder layer
                    # through the gated cross-attention, at the prompt pass and at every KV-cached step (no alignment loss in eval mode)
                    assert N_audio == B and [int(r) for r, _ in starts] == list(range(B)), "orca_hybrid: one audio per text row, in row order"
                    orca = self.orca
                    local16 = orca.local_forward(self.enc_all, N_audio) if cfg.orca_local_enabled else None
                    pc = self.llm._prompt_chunk(B)                            # chunked prompt pass: row buffers for one chunk (`begin_chunk`)
                    orca.begin(af, local16, B, S if pc is None else min(S, pc), None, False, keep_kv=True)
                    if orca.audio is not None:
                        hook, after = orca.inject, orca.begin_decode
                        chunk = orca.begin_chunk if pc is not None else None
                eos = eos_token_id if eos_token_id is not None else cfg.llm_config.eos_token_id
                if isinstance(eos, int):
                    eos = [eos]
                self._fwd = None
                lookup = None
                if self.llm.speculative:                                     # the lookup history: the ids the prompt embeds, -1 at pads and audio slots
                    lookup = src.view(B, S).to(torch.int64)
                    lookup = torch.where((attention_mask == 0) | (lookup < 0), torch.full_like(lookup, -1), lookup)
                extra = {}
                if constrained:                                              # the device tables, once per call
                    extra["constraints"] = ConstraintPlan(dev, eos, no_repeat_ngram_size, bad_words_ids, suppress_tokens, begin_suppress_tokens,
                                                          min_new_tokens)
                return self.llm.generate_greedy(fill, B, S, kv_start, int(max_new_tokens), int(pad_token_id), eos, draft_tokens=draft_tokens,
                                                lookup_ids=lookup,
                                                forced_tokens=forced_tokens, collect_logits=collect_logits, do_sample=bool(do_sample),
                                                temperature=1.0 if temperature is None else float(temperature),
                                                top_p=1.0 if top_p is None else float(top_p), seed=int(seed), layer_hook=hook, after_prompt=after,
                                                top_k=top_k, min_p=min_p, repetition_penalty=repetition_penalty,
                                                prompt_ids=(input_ids[:B // 2] if guided else input_ids) if prompt_in_history else None,
                                                chunk_hook=chunk, logprobs=logprobs, guidance_scale=guidance_scale, typical_p=typical_p,
                                                epsilon_cutoff=epsilon_cutoff, eta_cutoff=eta_cutoff, **extra)
        finally:
            self.training = was_training

    def hf_generation_kwargs(self, *, constraints: bool = False, truncation: bool = False, **explicit) -> dict:
        """`resolve_generation_kwargs(self.llm_generation_config, **explicit)`: the settings HF's `generate` would use for this
        checkpoint.  `model.generate(msgs, **model.hf_generation_kwargs(temperature=0.7, top_p=0.9, do_sample=True))` samples
        as the reference does (modeling_desta25.py:1419-1427), top_k from the checkpoint or HF's default 50 included.
        constraints=True: the checkpoint's no_repeat_ngram_size / bad_words_ids / suppress_tokens / begin_suppress_tokens /
        min_new_tokens come along for `generate` instead of raising.  truncation=True: so do its typical_p / epsilon_cutoff /
        eta_cutoff."""
        return resolve_generation_kwargs(self.llm_generation_config, constraints=constraints, truncation=truncation, **explicit)

    def _asr_whisper(self, waves) -> List[str]:
        """`perception.whisper.generate(input_features, attention_mask=None, max_new_tokens=128)` + `processor.batch_decode(...,
        skip_special_tokens=True)` (modeling_desta25.py:1580-1590) on the device: log-mel -> frozen encoder -> greedy decoder."""
        if getattr(self, "asr_tokenizer", None) is None:
            raise RuntimeError("ASR needs the Whisper tokenizer to turn token ids into text: model._setup_generation(asr_tokenizer=...) "
                               "(an object with batch_decode(ids, skip_special_tokens=True); no hub access to build one by name)")
        feats = self.processor(waves, sampling_rate=16000, return_tensors="pt").input_features
        ids = self.asr_decoder.generate(self.encoder, feats, max_new_tokens=128)
        self._last_asr_ids = ids
        return self.asr_tokenizer.batch_decode(ids.tolist(), skip_special_tokens=True)

    def _setup_generation(self, tokenizer=None, processor=None, vad=None, asr=None, asr_tokenizer=None):
        """The reference builds these from hub names (modeling_desta25.py:1465-1487): AutoTokenizer of the LLM (+ the audio locator
        token), the Whisper AutoProcessor, silero VAD from torch.hub and Whisper's own decoder for ASR.  Offline they are
        injected: `tokenizer` any object with the HF tokenizer call protocol, `processor` defaults to the device log-mel
        (`HipLogMelProcessor`), `vad(samples) -> truthy when the clip has speech` (default: every clip has speech), `asr(list of
        waveforms) -> list of str` (default: none — the Whisper DECODER is not on the hot path, so an audio with speech needs
        its "text" in the message)."""
        if tokenizer is not None:
            self.tokenizer = tokenizer
        if not hasattr(self, "tokenizer"):
            raise RuntimeError("generate() needs a tokenizer: model._setup_generation(tokenizer=...) (no hub access to build one by name)")
        tok = self.tokenizer
        tok.pad_token, tok.pad_token_id = tok.eos_token, tok.eos_token_id              # reference :1468-1469, unconditionally
        tok.padding_side = "left"
        if hasattr(tok, "add_tokens"):
            tok.add_tokens([self.audio_locator])
        assert len(tok.tokenize(self.audio_locator)) == 1, "audio_locator must be a single token"
        assert len(tok.tokenize(self.placeholder_token)) == 1, "placeholder_token must be a single token in the tokenizer"
        if processor is not None or not hasattr(self, "processor"):
            from ..utils.audio import HipLogMelProcessor
            self.processor = processor or HipLogMelProcessor(self.config.encoder_config.num_mel_bins, self.device)
        if vad is not None or not hasattr(self, "get_speech_timestamps"):
            self.get_speech_timestamps = vad
        if asr_tokenizer is not None or not hasattr(self, "asr_tokenizer"):
            self.asr_tokenizer = asr_tokenizer
            if asr_tokenizer is None and getattr(self, "asr_decoder", None) is not None and os.path.isdir(str(self.config.encoder_model_id)):
                try:                                                                     # the Whisper tokenizer files of the local checkpoint
                    from transformers import WhisperTokenizerFast
                    self.asr_tokenizer = WhisperTokenizerFast.from_pretrained(self.config.encoder_model_id, local_files_only=True)
                except Exception:                                                        # noqa: BLE001 — no tokenizer files: decode raises at use
                    self.asr_tokenizer = None
        if asr is not None or not hasattr(self, "asr"):
            self.asr = asr if asr is not None else (self._asr_whisper if getattr(self, "asr_decoder", None) is not None else None)

    check_logprobs_arg = staticmethod(check_logprobs_arg)

    def _logprob_fields(self, tok, ids, lp: TokenLogprobs, eos_ids) -> dict:
        """`GenerationOutput`'s log-prob fields from a `TokenLogprobs`: every row cut behind its first EOS (one host copy)."""
        tl, ti, tp = lp.token_logprobs.tolist(), lp.top_ids.tolist(), lp.top_logprobs.tolist()
        to_str = getattr(tok, "convert_ids_to_tokens", None)
        token_logprobs, top = [], []
        for b, row in enumerate(ids.tolist() if torch.is_tensor(ids) else ids):
            n = next((i + 1 for i, t in enumerate(row) if t in eos_ids), len(row))
            token_logprobs.append(tl[b][:n])
            top.append([[(i, to_str(i) if to_str is not None else None, v) for i, v in zip(ti[b][t], tp[b][t])] for t in range(n)])
        return dict(token_logprobs=token_logprobs, top_logprobs=top, sum_logprob=[float(sum(r)) for r in token_logprobs])

    def generate(self, messages, temperature=0.7, top_p=0.9, do_sample=True, max_new_tokens=512, seed=0, top_k=None, min_p=None,
                 repetition_penalty=None, logprobs=None, guidance_scale=None, negative_messages=None, no_repeat_ngram_size=None,
                 bad_words_ids=None, suppress_tokens=None, begin_suppress_tokens=None, min_new_tokens=None, typical_p=None,
                 epsilon_cutoff=None, eta_cutoff=None):
        """The reference's chat-level `generate` (modeling_desta25.py:1491-1721): messages -> audio decode -> log-mel -> placeholder
        expansion of every `<|AUDIO|>` -> left-padded tokenisation, pad-shifted start positions, transcription ids ->
        `_generate_step` -> `GenerationOutput(text, audios, generated_ids)`.  Same messages schema, same errors; the front-end
        models (tokenizer / VAD / ASR) are injected through `_setup_generation`.  top_k / min_p / repetition_penalty: HF's
        processors of the same names, None = off (see `_generate_step`).  To sample exactly as the reference's
        `llm_model.generate` does, with the checkpoint's generation_config.json and HF's defaults (top_k = 50) filled in:
        `model.generate(msgs, **model.hf_generation_kwargs(temperature=0.7, top_p=0.9, do_sample=True))`.
        logprobs = n (0..32): the output also carries `token_logprobs`, `top_logprobs` (n alternatives per token) and `sum_logprob`,
        each row cut behind its first EOS — the model's own distribution, log_softmax of the raw logits in front of the penalty,
        the temperature and the filters (HF's output_logits, not output_scores).
        guidance_scale = g (None or 1: off): classifier-free guidance, HF's `guidance_scale` with a negative prompt
        (UnbatchedClassifierFreeGuidanceLogitsProcessor): every step's scores are g * (lc - lu) + lu, lc / lu the log-softmax under
        the prompt and under the negative prompt, in front of the penalty, temperature and filters.  `negative_messages`: one
        conversation per conversation of `messages`; None: the same chat without its audio (`guidance_negative_messages`), which
        pushes the answer towards what the audio says (audio-contrastive decoding).  Both run as one left-padded batch of twice
        the rows; the output has one row per conversation of `messages` and lists their audios only.
        no_repeat_ngram_size / bad_words_ids / suppress_tokens / begin_suppress_tokens / min_new_tokens: HF's hard constraints of
        the same names, None = off (see `_generate_step`): no n-gram of that size twice, the listed token sequences / tokens never
        (the listed begin tokens not as the first token), no EOS before m new tokens.  An audio chat matches them against the
        answer alone, a text-only chat against prompt + answer, as HF does for `inputs_embeds` / `input_ids` prompts.  A
        checkpoint's own settings: `model.generate(msgs, **model.hf_generation_kwargs(constraints=True))`.
        typical_p / epsilon_cutoff / eta_cutoff: HF's truncation warpers of the same names behind min-p (locally typical sampling,
        epsilon and eta sampling), None = off, sampling only (see `_generate_step`).  A checkpoint's own:
        `model.hf_generation_kwargs(truncation=True)`."""
        check_sampling_args(top_k, min_p, repetition_penalty)
        check_truncation_args(typical_p, epsilon_cutoff, eta_cutoff)
        check_logprobs_arg(logprobs)
        check_guidance_arg(guidance_scale)
        cons = dict(no_repeat_ngram_size=no_repeat_ngram_size, bad_words_ids=bad_words_ids, suppress_tokens=suppress_tokens,
                    begin_suppress_tokens=begin_suppress_tokens, min_new_tokens=min_new_tokens)
        check_constraint_args(**cons, vocab=getattr(getattr(self, "llm", None), "V", None))
        extra = dict(top_k=top_k, min_p=min_p, repetition_penalty=repetition_penalty)
        extra.update({k: v for k, v in cons.items() if v is not None})
        extra.update({k: v for k, v in dict(typical_p=typical_p, epsilon_cutoff=epsilon_cutoff, eta_cutoff=eta_cutoff).items() if v is not None})
        if logprobs is not None:
            extra["logprobs"] = logprobs
        if guidance_scale is not None and float(guidance_scale) != 1.0:
            if not isinstance(messages, list) or not messages:
                raise ValueError("messages should be a list of dictionaries or a list of lists.")
            conversations = [messages] if isinstance(messages[0], dict) else list(messages)
            n_audio = sum(len(m.get("audios", [])) for conv in conversations for m in conv)
            if negative_messages is None:
                if n_audio == 0:
                    raise ValueError("guidance_scale: the chat has no audio, so the derived negative prompt would be the prompt itself: pass negative_messages")
                negatives = guidance_negative_messages(conversations, self.audio_locator)
            else:
                negatives = [negative_messages] if negative_messages and isinstance(negative_messages[0], dict) else list(negative_messages)
            if len(negatives) != len(conversations):
                raise ValueError(f"guidance_scale: negative_messages holds {len(negatives)} conversations for {len(conversations)} of messages")
            extra["guidance_scale"] = guidance_scale
            tok, inputs, audios, texts = self._chat_inputs(conversations + negatives)
            text_only = not audios
            audios, texts = audios[:n_audio], texts[:n_audio]                # the conditional conversations' (they come first)
        else:
            tok, inputs, audios, texts = self._chat_inputs(messages)
            text_only = not audios
        if text_only:
            # no audio: plain LLM generation on the chat template; stops on eos or <|eot_id|>
            eos = [tok.eos_token_id, tok.convert_tokens_to_ids("<|eot_id|>")]
            ids = self._generate_step(inputs, pad_token_id=tok.pad_token_id, temperature=temperature, top_p=top_p, max_new_tokens=max_new_tokens,
                                      do_sample=do_sample, eos_token_id=eos, seed=seed, prompt_in_history=True, **extra)
            lp = {}
            if logprobs is not None:
                ids, tlp = ids
                lp = self._logprob_fields(tok, ids, tlp, eos)
            rows = [r.tolist() for r in ids]
            return GenerationOutput(text=tok.batch_decode(rows, skip_special_tokens=True), audios=[], generated_ids=rows, **lp)
        self._last_generate_inputs = inputs
        ids = self._generate_step(inputs, pad_token_id=tok.pad_token_id, temperature=temperature, top_p=top_p, max_new_tokens=max_new_tokens,
                                  do_sample=do_sample, seed=seed, **extra)
        lp = {}
        if logprobs is not None:
            ids, tlp = ids
            eos = self.config.llm_config.eos_token_id
            lp = self._logprob_fields(tok, ids, tlp, [eos] if isinstance(eos, int) else list(eos or []))
        return GenerationOutput(text=tok.batch_decode(ids, skip_special_tokens=True), audios=list(zip(audios, texts)), generated_ids=ids.tolist(), **lp)

    def _chat_inputs(self, messages):
        """The front half of the reference's chat-level `generate` (modeling_desta25.py:1491-1700), shared by `generate` and
        `score`: chat template with the generation prompt, audio decode, VAD / ASR rules, log-mel, `<start_audio>` / `<end_audio>`
        indicator, placeholder expansion, left-padded tokenisation, pad-shifted start positions, transcription ids.
        -> (tokenizer, `_generate_step` inputs, audios, texts); a chat without audio has no features and no spans."""
        from ..trainer.data.simple_dataset import prepare_audio_context_and_start_positions
        from ..utils.audio import AudioSegment
        if not hasattr(self, "tokenizer") or not hasattr(self, "processor"):
            self._setup_generation()
        tok = self.tokenizer
        if not isinstance(messages, list):
            raise ValueError("messages should be a list of dictionaries or a list of lists.")
        conversations = [messages] if isinstance(messages[0], dict) else messages
        audios, texts = [], []
        for conv in conversations:
            for m in conv:
                au = m.get("audios", [])
                assert len(au) == m["content"].count(self.audio_locator), "audio count does not match (<|AUDIO|>) count"
                audios += [a["audio"] for a in au]
                texts += [a.get("text") for a in au]
        if not audios:
            enc = tok(tok.apply_chat_template(conversations, tokenize=False, add_generation_prompt=True), return_tensors="pt", padding=True)
            inputs = {"context_input_ids": enc["input_ids"], "context_attention_mask": enc["attention_mask"],
                      "context_batch_start_positions": [], "batch_transcription_ids": [], "batch_features": None}
            return tok, inputs, audios, texts
        waves, need_asr = [], []
        for i, (a, t) in enumerate(zip(audios, texts)):
            if isinstance(a, str) and not os.path.exists(a):
                raise ValueError(f"Audio file {a} does not exist.")
            w = AudioSegment.from_file(a, target_sr=16000, channel_selector="average").samples
            waves.append(w)
            speech = True if self.get_speech_timestamps is None else bool(self.get_speech_timestamps(w))
            if speech and t is None:
                need_asr.append(i)
            if not speech:
                texts[i] = " "
        if need_asr:
            if self.asr is None:
                raise NotImplementedError("an audio with speech and no 'text' needs ASR: the Whisper checkpoint in use carries no decoder "
                                          "weights (model.decoder.*) — pass the transcription in the message or inject asr= through _setup_generation")
            for i, t in zip(need_asr, self.asr([waves[i] for i in need_asr])):
                texts[i] = t.strip()
        feats = self.processor(waves, sampling_rate=16000, return_tensors="pt").input_features
        n = len(waves)
        audio_sizes, tr_sizes = [getattr(self.config, "audio_tokens", self.config.prompt_size)] * n, [len(tok.tokenize(t, add_special_tokens=False)) for t in texts]       # (:1574-1578)
        contexts, starts = [], []
        for conv in conversations:
            ctx = tok.apply_chat_template(conv, tokenize=False, add_generation_prompt=True)
            ctx = ctx.replace(self.audio_locator, f"<start_audio>{self.audio_locator}<end_audio>")      # the training-time indicator
            toks, st = prepare_audio_context_and_start_positions(tok.tokenize(ctx), self.audio_locator, audio_sizes, tr_sizes, self.placeholder_token)
            contexts.append(tok.convert_tokens_to_string(toks))
            starts.append(st)
        enc = tok(contexts, truncation=True, padding="longest", return_tensors="pt", return_length=True, add_special_tokens=False)
        pad = torch.as_tensor(enc["length"], dtype=torch.long) - enc["attention_mask"].sum(dim=1)
        inputs = {"batch_features": feats,
                  "batch_transcription_ids": [tok.encode(t, add_special_tokens=False, return_tensors="pt").long() for t in texts],
                  "context_input_ids": enc["input_ids"], "context_attention_mask": enc["attention_mask"],
                  "context_batch_start_positions": [(i, s + pad[i]) for i in range(len(starts)) for s in starts[i]]}
        return tok, inputs, audios, texts

    # -- scoring: token log-probabilities ------------------------------------------------------------------------
    @torch.no_grad()
    def score_batch(self, input_ids, attention_mask, batch_features, batch_transcription_ids, batch_start_positions, labels, **kwargs) -> ScoreOutput:
        """Log-likelihood of every row's target tokens (labels != -100 after the causal shift): `forward`'s inputs, in eval mode
        (no Q-Former dropout; the training flag is restored) and without gradients.  The prefill runs once with the lm_head on
        the target rows only (`desta_target_rows`, batch-major grid), the loss kernel reads those compact logits without
        writing a gradient, and `desta_token_logprobs` reads them again for the per-token values; a row's tokens are one
        contiguous segment of the compact list, summed in a fixed order, so two calls agree bit for bit.  Scoring runs the
        prefill kernels on the bf16 weights: `set_decode_weights("fp8")` changes the KV-cached decode steps only, not this.
        ORCA: the auxiliary losses of the forward are computed once and are not part of `loss` (the LM loss, as `forward`)."""
        if labels is None:
            raise ValueError("score_batch() needs labels: they select the tokens to score")
        B, S = input_ids.shape
        was_training = self.training
        self.training = False
        try:
            out = self.forward(input_ids, attention_mask, batch_features, batch_transcription_ids, batch_start_positions, labels=labels,
                               compact_targets=True, **kwargs)
            dev = self.device
            lab = labels.detach().to("cpu")
            n_host = (lab[:, 1:] != -100).sum(dim=1)                               # row (b, s) predicts labels[b, s + 1]
            n_list = [int(n) for n in n_host.tolist()]
            _, lab_c, Mc = self.llm.compact
            assert Mc == sum(n_list), "compact target rows do not match the labels"
            with torch.cuda.device(dev):
                lp = torch.zeros(Mc, dtype=F32, device=dev)
                top = torch.zeros(Mc, dtype=torch.uint8, device=dev)
                if Mc > 0:
                    # compact row i predicts lab_c[1 + i] (the layout desta_causal_lm_loss(batch = 1) consumes, shifted by one)
                    H.token_logprobs(self.llm.logits, self.llm.Vp, lab_c[1:], Mc, self.config.llm_config.vocab_size, lp, top)
                n_tokens = n_host.to(dev)
                # segments of the compact list -> [B, longest] (zero padded), one fixed-order sum per row
                T = max(n_list) if n_list else 0
                seg = torch.arange(T, device=dev).unsqueeze(0) < n_tokens.unsqueeze(1)
                lp_pad = torch.zeros(B, T, dtype=F32, device=dev)
                top_pad = torch.zeros(B, T, dtype=torch.int64, device=dev)
                lp_pad[seg] = lp
                top_pad[seg] = top.to(torch.int64)
                return ScoreOutput(sum_logprob=lp_pad.sum(dim=1), n_tokens=n_tokens, token_logprobs=list(torch.split(lp, n_list)),
                                   top1_match=top_pad.sum(dim=1), loss=out.loss)
        finally:
            self.training = was_training

    def score(self, messages, choices, normalize="sum") -> ChoiceScores:
        """Rank answer options by their log-likelihood as the assistant's reply to ONE conversation (`generate`'s messages schema,
        with or without audios): the context is built exactly as `generate` builds it (`_chat_inputs`), every choice's token ids
        (`add_special_tokens=False`) and the tokenizer's EOS are appended, rows are left-padded to a common length and only the
        choice tokens and the EOS carry labels.  Each audio is decoded, log-mel'd and encoded ONCE: every row's audio span
        points at the same connector output rows.  normalize: "sum" (log-likelihood) or "mean" (per token, length-normalised)."""
        check_score_args(choices, normalize)
        tok, inputs, audios, _ = self._chat_inputs(messages)
        ctx_ids, ctx_mask = inputs["context_input_ids"], inputs["context_attention_mask"]
        if ctx_ids.shape[0] != 1:
            raise ValueError("score() takes one conversation")
        ctx = ctx_ids[0][ctx_mask[0].bool()].tolist()
        pad0 = int(ctx_ids.shape[1]) - len(ctx)
        tails = []
        for c in choices:
            ids = tok.encode(c, add_special_tokens=False)
            ids = ids[0].tolist() if torch.is_tensor(ids) else list(ids)
            if not ids:
                raise ValueError(f"choice {c!r} has no tokens")
            tails.append(ids + [int(tok.eos_token_id)])
        n, S = len(tails), len(ctx) + max(len(t) for t in tails)
        input_ids = torch.full((n, S), int(tok.pad_token_id), dtype=torch.long)
        attention_mask = torch.zeros(n, S, dtype=torch.long)
        labels = torch.full((n, S), -100, dtype=torch.long)
        starts, trs, audio_index = [], [], []
        for i, t in enumerate(tails):
            pad = S - len(ctx) - len(t)
            input_ids[i, pad:] = torch.tensor(ctx + t)
            attention_mask[i, pad:] = 1
            labels[i, S - len(t):] = torch.tensor(t)
            for a, (_, s0) in enumerate(inputs["context_batch_start_positions"]):
                starts.append((i, int(s0) - pad0 + pad))
                trs.append(inputs["batch_transcription_ids"][a])
                audio_index.append(a)
        extra = dict(audio_index=audio_index) if audios else {}
        out = self.score_batch(input_ids, attention_mask, inputs["batch_features"], trs, starts, labels, **extra)
        scores = out.sum_logprob if normalize == "sum" else out.sum_logprob / out.n_tokens.to(F32)
        return ChoiceScores(scores=scores, best=int(scores.argmax()), token_logprobs=out.token_logprobs, n_tokens=out.n_tokens)

    def _target_rows(self, labels, B: int, S: int, s_major: bool = False):
        """Index list / compact labels / host-visible count of the rows that carry a target, on a side stream: it waits for
        the main stream's current position (the producer of `labels`), runs one tiny kernel and copies the count to pinned
        memory; the main stream's later work is not involved, so synchronising on the event at lm_head time does not drain it."""
        dev = self.device
        if self._tr_stream is None:
            self._tr_stream = torch.cuda.Stream(device=dev)
            self._tr_count_host = torch.zeros(2, dtype=torch.int32).pin_memory()     # (rows with a target, first position with a target)
        M = B * S
        if self._tr_idx is None or self._tr_idx.numel() < M:
            self._tr_idx = torch.empty(M, dtype=torch.int32, device=dev)
            self._tr_lab = torch.empty(M + 2, dtype=torch.int64, device=dev)
            self._tr_count = torch.zeros(2, dtype=torch.int32, device=dev)
        main = torch.cuda.current_stream(dev)
        lab_dev = labels.to(dev).contiguous()
        self._tr_labels_keep = lab_dev                                           # alive until the side stream has read it
        self._tr_stream.wait_stream(main)
        with torch.cuda.stream(self._tr_stream):
            H.target_rows(lab_dev, B, S, self._tr_idx, self._tr_lab, self._tr_count, s_major=s_major)
            self._tr_count_host.copy_(self._tr_count, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self._tr_stream)
        main.wait_stream(self._tr_stream)                                        # idx / compact labels are read on the main stream
        return self._tr_idx, self._tr_lab, self._tr_count_host, ev

    def _enc_buf(self, idx: int, N: int) -> torch.Tensor:
        e, nt = self.config.encoder_config, len(self.config.target_layer_ids)
        b = self._enc_bufs[idx]
        if b is None or b.shape[1] != N * e.max_source_positions:
            b = self._enc_bufs[idx] = torch.empty(nt, N * e.max_source_positions, e.d_model, dtype=BF16, device=self.device)
        return b

    def drop_prefetched(self) -> None:
        """Forget prefetched encoder outputs (their batches will never run); the encoder's scratch is free again afterwards."""
        main = torch.cuda.current_stream(self.device)
        for pf in self._enc_pending:
            if pf[4] is not None:
                main.wait_event(pf[4])
        self._enc_pending = []

    def _encode(self, batch_features: torch.Tensor, N: int) -> None:
        """self.enc_all := tapped Whisper states of `batch_features`: the prefetched ones when `prefetch_encoder` ran for this
        very tensor OBJECT, unmodified since (a new tensor can reuse a freed tensor's address and shape, so data_ptr / shape
        keys could alias a stale encoder output), else computed now."""
        main = torch.cuda.current_stream(self.device)
        for k, pf in enumerate(self._enc_pending):
            if pf[0] is batch_features and pf[1] == batch_features._version and pf[2] == N:
                if pf[4] is not None:
                    main.wait_event(pf[4])
                del self._enc_pending[k]                 # a prefetch for the batch AFTER this one may stay pending
                self._enc_cur = pf[3]
                self.enc_all = self._enc_bufs[self._enc_cur]
                return
        # miss: the encoder's scratch buffers are shared with any prefetch still running -> wait for all of them
        busy = {pf[3] for pf in self._enc_pending}
        for pf in self._enc_pending:
            if pf[4] is not None:
                main.wait_event(pf[4])
        if len(busy) > 1:                                # both buffers hold prefetched batches that are not this one: stale
            self._enc_pending, busy = [], set()
        if self._enc_cur in busy:
            self._enc_cur = 1 - self._enc_cur
        self.enc_all = self._enc_buf(self._enc_cur, N)
        self.encoder.forward(batch_features.to(self.device, F32).contiguous(), self.enc_all)

    def prefetch_encoder(self, batch_features: torch.Tensor, stream: Optional["torch.cuda.Stream"] = None) -> None:
        """Run the FROZEN Whisper encoder for a LATER batch now, into the tapped-state buffer no pending batch occupies.  It
        depends on nothing the optimizer writes, so with `stream` it runs on that HIP stream from the current position of the
        calling stream on, CONCURRENTLY with whatever the calling stream does next (the LLM forward / backward of the current
        batch: its VALU-bound attention, HBM-bound norms and partial GEMM rounds fill in beside the MFMA-bound LLM GEMMs); the
        consumer waits on its event in `_encode`.  Without `stream` it runs in line on the current stream.  At most one
        consumed-later batch besides the current one is kept (two buffers)."""
        dev = self.device
        N = batch_features.shape[0]
        with torch.cuda.device(dev):
            main = torch.cuda.current_stream(dev)
            if len(self._enc_pending) >= 2:
                self.drop_prefetched()
            # the buffer of the batch consumed LAST (its backward is already queued on the calling stream) unless a pending
            # prefetch sits there; the one in flight for the current batch keeps the other
            busy = {pf[3] for pf in self._enc_pending}
            idx = (1 - next(iter(busy))) if busy else 1 - self._enc_cur
            for pf in self._enc_pending:                 # one encoder at a time on the shared scratch: order behind the pending one
                if pf[4] is not None:
                    (stream or main).wait_event(pf[4])
            buf = self._enc_buf(idx, N)
            mel = batch_features.to(dev, F32).contiguous()
            ev = None
            if stream is None:
                self.encoder.forward(mel, buf)
            else:
                stream.wait_stream(main)                 # inputs ready; the buffer's last reader (a finished batch's backward) queued
                with torch.cuda.stream(stream):
                    self.encoder.forward(mel, buf)
                    ev = torch.cuda.Event()
                    ev.record(stream)
                self._enc_keep = mel
        self._enc_pending.append((batch_features, batch_features._version, N, idx, ev))

    def backward(self) -> None:
        """Gradients of the last forward's loss w.r.t. every connector tensor -> arena.grads (overwritten)."""
        self.backward_connector(self.backward_llm())

    def backward_connector(self, d_af: torch.Tensor) -> None:
        """Second half of `backward`: d_af = dL/d audio_features -> every connector gradient.  Its ~600 small launches (2048-row
        GEMMs, LayerNorms, cross-attention) leave most of the chip idle, and nothing of the NEXT batch's frozen Whisper forward
        depends on them: the trainer runs this half on its side stream beside that forward (`overlap_comm`)."""
        with torch.cuda.device(self.device):
            if d_af is None:                       # use_lora, batch without audio: `backward_llm` zeroed the connector's gradients
                return
            self.connector.backward(d_af)

    def backward_llm(self) -> torch.Tensor:
        """First half of `backward`: dX through the frozen LLM down to the audio rows; returns dL/d audio_features [N_audio*K, h]."""
        f = self._fwd
        if f and f.get("orca") and f["has_grad"]:
            # gradient of the trainer's total loss = LM loss + sum of the ORCA losses (desta_trainer.py:56-92)
            K, S, B = self.audio_tokens, f["S"], f["B"]
            with torch.cuda.device(self.device):
                self.arena.grads.zero_()
                self.orca.begin_backward()
                dx0 = self.llm.backward(layer_hook_bwd=self.orca.inject_bwd)
                idx = self._audio_slots(f["starts"], B, S, False)[2]
                d_af = torch.empty(f["N_audio"] * K, self.config.llm_config.hidden_size, dtype=BF16, device=self.device)
                H.gather_rows(dx0, idx, f["N_audio"] * K, self.config.llm_config.hidden_size, d_af)
                self.orca.backward_tail(d_af)
            self._fwd = None
            return None
        if not f or not f["has_grad"]:
            raise RuntimeError("backward() needs a training-mode forward with labels and at least one audio")
        K, S, B = self.config.prompt_size, f["S"], f["B"]
        with torch.cuda.device(self.device):
            if f["s_major"] and f["starts"]:
                dx0 = self.llm.backward(first_needed_pos=min(s for _, s in f["starts"]),
                                        out_rows=(min(s for _, s in f["starts"]), max(s for _, s in f["starts"]) + K))
            else:
                dx0 = self.llm.backward()
            if f["N_audio"] == 0:                  # use_lora, batch without audio: only the adapters have a gradient
                end = min((self.arena.offsets[n] for n in self.arena.names if ".lora_" in n), default=self.arena.numel)
                self.arena.grads[:end].zero_()
                self._fwd = None
                return None
            idx = self._audio_slots(f["starts"], B, S, f["s_major"])[2]
            d_af = torch.empty(f["N_audio"] * K, self.config.llm_config.hidden_size, dtype=BF16, device=self.device)
            H.gather_rows(dx0, idx, f["N_audio"] * K, self.config.llm_config.hidden_size, d_af)
        self._fwd = None
        return d_af
