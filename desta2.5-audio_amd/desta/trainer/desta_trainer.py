"""Training loop of the MI355X-native DeSTA2.5 path.

Mirrors the reference's `DeSTA25Trainer(transformers.Trainer)` (desta/trainer/desta_trainer.py:33-102)
and the slice of the HF loop it inherits (TF:trainer.py:1722-1800): per optimizer step
    forward -> loss -> backward -> [DDP mean of gradients] -> clip_grad_norm_(1.0) -> Adafactor
    -> linear-warmup scheduler step -> zero_grad
with `compute_loss` keeping the reference's signature / empty-batch guard / log keys.  Differences that
are the point of the rewrite: gradients are ONE flat fp32 arena (one RCCL all-reduce, no buckets), the
optimizer is 6 fused launches, per-step logging keeps device scalars (no `.item()` host sync on the
hot path; values are materialised every `logging_steps`), and the gradient exchange + optimizer of
step t run on a side HIP stream concurrently with the frozen Whisper forward of step t+1.
"""
from __future__ import annotations

import json
import logging
import math
import os
from dataclasses import dataclass
from typing import Any, Dict, Iterable, List, Optional

import torch
import torch.distributed as dist

from ..models.modeling_desta25 import DeSTA25AudioModel
from ..optim import FusedAdafactor, FusedAdamW, linear_warmup_lr


@dataclass
class TrainingArguments:
    """The subset of `transformers.TrainingArguments` that `train_desta.py:133-162` sets."""
    output_dir: str = "./exp"
    learning_rate: float = 1e-4
    weight_decay: float = 0.01
    warmup_steps: int = 5000
    max_steps: int = -1
    num_train_epochs: float = 1.0
    per_device_train_batch_size: int = 8
    per_device_eval_batch_size: int = 8
    gradient_accumulation_steps: int = 1
    max_grad_norm: float = 1.0
    logging_steps: int = 10
    optim: str = "adafactor"                       # | "adamw_torch" | "adamw_torch_fused" (HF: both torch.optim.AdamW, TF:trainer_optimizer.py:201-208)
    adam_beta1: float = 0.9                        # HF TrainingArguments defaults; used by the AdamW optimizers only
    adam_beta2: float = 0.999
    adam_epsilon: float = 1e-8
    bf16: bool = True
    overlap_comm: bool = True
    overlap_connector_backward: bool = False       # with overlap_comm: the connector's backward ALSO runs on the side stream (bit-identical results; round 3: -0.4 ms WITHOUT the encoder stream; round 4, beside `overlap_encoder`: +0.5 ms and 4x the step-time spread, same-box A/B -> off)
    overlap_encoder: bool = True                   # next batch's frozen Whisper forward on its own HIP stream beside the connector / LLM of the current batch (bit-identical results; default since round 4)
    side_stream_priority: int = 0                  # HIP priority of the encoder-prefetch and optimizer-tail streams.  gfx950 offers (least, greatest) = (0, -1): nothing BELOW the default stream's 0 exists, so the side work cannot be demoted; promoting the main work instead (the whole step on a priority -1 stream, `bench.py --main-priority -1`) measured -0.5 ms (0.3 %) and is not shipped (every caller of the trainer would have to order its own default-stream work against that stream)
    save_strategy: str = "no"                      # "epoch" (train_desta.py:146, enable_checkpointing) | "no"
    steps_per_epoch: Optional[int] = None          # len(train dataloader) = MICRO-batches per epoch when the dataset is not sized (synthetic streams)
    eval_strategy: str = "no"                      # "steps" (every eval_steps optimizer steps) | "epoch" | "no" (train_desta.py:147-148)
    eval_steps: Optional[int] = None
    dataloader_num_workers: int = 0                # `dataset.train_ds.num_workers` (train_desta.py:158): worker PROCESSES running the collate's host half (decode, resample, tokenise)
    dataloader_pin_memory: bool = True             # `dataset.train_ds.pin_memory` (train_desta.py:159): the loader pins the tensors the workers hand over
    dataloader_prefetch_factor: int = 2            # batches in flight per worker (torch DataLoader default)
    seed: int = 42                                 # map-style datasets: the epoch's sample order is randperm(seed + epoch)
    shuffle: bool = True                           # (HF: RandomSampler unless group_by_length); False = manifest order


OPTIMIZERS = ("adafactor", "adamw_torch", "adamw_torch_fused")        # values of `TrainingArguments.optim` this trainer runs

ALLREDUCE_CALLS: Dict[str, int] = {}              # "<backend>:<op>" -> collectives issued by this process (tests assert which branch ran)


def allreduce_mean_(flat: torch.Tensor) -> None:
    """Mean over data-parallel ranks of ONE flat buffer (what DDP's bucketed reducer does for the
    reference, accelerate `accelerator.py:1892`): RCCL AVG over xGMI on GPUs, SUM + scale on gloo."""
    if not (dist.is_available() and dist.is_initialized()):
        return
    if dist.get_world_size() == 1 and not os.environ.get("DESTA_ALLREDUCE_WORLD1"):      # (set by `bench.py --force-dist`: rehearsal of the collective on one GPU)
        return
    if dist.get_backend() == "nccl":
        dist.all_reduce(flat, op=dist.ReduceOp.AVG)
        ALLREDUCE_CALLS["nccl:AVG"] = ALLREDUCE_CALLS.get("nccl:AVG", 0) + 1
    else:
        dist.all_reduce(flat, op=dist.ReduceOp.SUM)
        flat.mul_(1.0 / dist.get_world_size())
        key = f"{dist.get_backend()}:SUM*1/world"
        ALLREDUCE_CALLS[key] = ALLREDUCE_CALLS.get(key, 0) + 1


def micro_batches_per_epoch(args: TrainingArguments, n_samples: Optional[int], world: int) -> Optional[int]:
    """len(train dataloader) of one rank: `args.steps_per_epoch` for unsized (synthetic) streams, else
    ceil(ceil(N / world) / per_device_batch) (DistributedSampler pads every rank to an equal share)."""
    if args.steps_per_epoch is not None:
        return max(1, int(args.steps_per_epoch))
    if n_samples is None:
        return None
    return max(1, math.ceil(math.ceil(n_samples / world) / args.per_device_train_batch_size))


def steps_per_epoch(args: TrainingArguments, n_samples: Optional[int], world: int) -> Optional[int]:
    """OPTIMIZER steps per epoch as HF derives them (TF:trainer.py:2356-2360 `set_initial_training_values`):
    len(dataloader) // GA + (1 if len(dataloader) % GA else 0) — the last window of an epoch may hold fewer micro-batches
    (TF:trainer.py:1715-1725 `remainder`); windows never straddle an epoch boundary."""
    mb = micro_batches_per_epoch(args, n_samples, world)
    if mb is None:
        return None
    ga = max(1, args.gradient_accumulation_steps)
    return max(1, mb // ga + (1 if mb % ga else 0))


def resolve_total_steps(args: TrainingArguments, spe: Optional[int]) -> int:
    """`num_training_steps` handed to get_linear_schedule_with_warmup: max_steps if positive (it takes precedence over epochs),
    else ceil(num_train_epochs * steps_per_epoch).  Every shipped full-size YAML uses max_steps: -1 with max_epochs: 5."""
    if args.max_steps > 0:
        return int(args.max_steps)
    if spe is None:
        raise ValueError("args.max_steps must be set to a positive value if dataloader does not have a length, "
                         f"was {args.max_steps}")                              # the HF Trainer's own message
    return max(1, math.ceil(args.num_train_epochs * spe))


class DeSTA25Trainer:
    def __init__(self, model: DeSTA25AudioModel, cfg: Any = None, args: Optional[TrainingArguments] = None,
                 train_dataset=None, eval_dataset=None, data_collator=None, processing_class=None, **kwargs):
        self.model, self.cfg, self.args = model, cfg, args or TrainingArguments()
        self.train_dataset, self.eval_dataset, self.data_collator = train_dataset, eval_dataset, data_collator
        self.processing_class = processing_class
        from ..utils.metrics import ConsecutiveWordsAccuracyMetric
        self.metrics = ConsecutiveWordsAccuracyMetric()                       # desta_trainer.py:36
        if self.args.optim not in OPTIMIZERS:
            raise NotImplementedError(f"optim={self.args.optim!r} is not implemented (choose one of {', '.join(OPTIMIZERS)})")
        if self.args.gradient_accumulation_steps < 1:
            raise ValueError("gradient_accumulation_steps must be >= 1")
        self._micro, self._acc = 0, None                                      # micro-batches seen in the current accumulation window / their gradient sum
        if self.args.optim == "adafactor":
            self.optimizer = FusedAdafactor(model.arena, weight_decay=self.args.weight_decay, max_grad_norm=self.args.max_grad_norm)
        else:
            self.optimizer = FusedAdamW(model.arena, weight_decay=self.args.weight_decay,
                                        betas=(self.args.adam_beta1, self.args.adam_beta2), eps=self.args.adam_epsilon,
                                        max_grad_norm=self.args.max_grad_norm, torch_fused=self.args.optim == "adamw_torch_fused")
        self.global_step = 0
        self._total_steps: Optional[int] = None
        self.world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        self.rank = dist.get_rank() if self.world > 1 else 0
        model.dropout_seed = 1 + self.rank                                    # ranks draw different dropout masks (as under DDP)
        pr = int(self.args.side_stream_priority)
        self._side = torch.cuda.Stream(device=model.device, priority=pr) if self.args.overlap_comm else None
        self._enc_stream = torch.cuda.Stream(device=model.device, priority=pr) if self.args.overlap_encoder else None
        self._side_done: Optional[torch.cuda.Event] = None
        self._log_buffer: List[Dict[str, Any]] = []
        self.log_history: List[Dict[str, float]] = []
        self.prediction_step_outputs: List[Dict[str, Any]] = []
        self._apply_decode_rows(model, cfg)

    @staticmethod
    def _apply_decode_rows(model, cfg: Any) -> Optional[int]:
        """`trainer.decode_rows: n` of the config: the row ceiling of evaluate()'s KV-cached steps (`model.set_decode_rows`; absent or
        null: the model keeps its setting).  Returns what it set."""
        tr = (cfg.get("trainer") if hasattr(cfg, "get") else getattr(cfg, "trainer", None)) if cfg is not None else None
        rows = (tr.get("decode_rows") if hasattr(tr, "get") else getattr(tr, "decode_rows", None)) if tr is not None else None
        if rows is not None:
            model.set_decode_rows(rows)
        return rows

    def steps_per_epoch(self) -> Optional[int]:
        ds = self.train_dataset
        return steps_per_epoch(self.args, len(ds) if ds is not None and hasattr(ds, "__len__") else None, self.world)

    @property
    def total_steps(self) -> int:
        if self._total_steps is None:
            self._total_steps = resolve_total_steps(self.args, self.steps_per_epoch())
        return self._total_steps

    @total_steps.setter
    def total_steps(self, v: int) -> None:
        self._total_steps = int(v)

    # -- reference surface ---------------------------------------------------------------------
    def _is_empty_batch(self, inputs: Dict[str, Any]) -> bool:
        return inputs.get("_empty_batch", False)

    def get_last_lr(self) -> float:
        return linear_warmup_lr(self.global_step, self.args.learning_rate, self.args.warmup_steps, self.total_steps)

    def compute_loss(self, model: DeSTA25AudioModel, inputs: Dict[str, Any], return_outputs: bool = False, **kwargs):
        """desta_trainer.py:43-102 (qformer_1 branch).  `num_items_in_batch` is swallowed by **kwargs,
        so the loss stays the per-rank token mean (hazard H8)."""
        if self._is_empty_batch(inputs):
            logging.warning("Skipping empty batch (audio decode errors)")
            zero = torch.zeros((), device=model.device)
            return (zero, None) if return_outputs else zero
        outputs = model(**inputs)
        lm_loss = outputs.loss
        total_loss = lm_loss
        # device scalars only: materialised in `_flush_logs` (the reference's 3 x .item() per step
        # serialise host and device every step, SURVEY §2.2 last row)
        log = {"train/lm_loss": lm_loss, "train/ppl": torch.exp(lm_loss)}
        orca = getattr(outputs, "orca_losses", None)
        if orca and getattr(getattr(model, "config", None), "connector_mode", "") == "orca_hybrid":
            # desta_trainer.py:67-92: every ORCA auxiliary loss is added to the LM loss (already weighted) and logged under its name
            orca_total = None
            for name, l in orca.items():
                if l is not None:
                    total_loss = total_loss + l
                    orca_total = l if orca_total is None else orca_total + l
                    log[f"train/{name}"] = l
            if orca_total is not None:
                log["train/orca_total"] = orca_total
        log["train/loss"] = total_loss
        log["train/learning_rate"] = self.get_last_lr()
        self.log(log)
        return (total_loss, outputs) if return_outputs else total_loss

    def log(self, d: Dict[str, Any]) -> None:
        self._log_buffer.append({k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in d.items()})
        if len(self._log_buffer) >= max(1, self.args.logging_steps):
            self._flush_logs()

    def _flush_logs(self) -> None:
        for d in self._log_buffer:
            self.log_history.append({k: (float(v) if torch.is_tensor(v) else v) for k, v in d.items()})
        self._log_buffer.clear()

    # -- one optimizer step ----------------------------------------------------------------------
    def _reduce_and_update(self, lr: float) -> None:
        arena = self.model.arena
        prof = getattr(self, "comm_profile", None)
        if prof is not None:                                                  # bench.py: HIP events around the collective, on the stream it runs on
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            allreduce_mean_(arena.grads)
            e1.record()
            prof.append(("allreduce", e0, e1))
        else:
            allreduce_mean_(arena.grads)                                      # one flat buffer, no buckets
        self.optimizer.step(lr)
        self.model.refresh_weights()

    def wait_update(self) -> None:
        """Main stream waits for the side-stream all-reduce + optimizer of the previous step."""
        if self._side_done is not None:
            main = torch.cuda.current_stream(self.model.device)
            prof = getattr(self, "comm_profile", None)
            if prof is not None:                                              # how long the main stream sits in front of this wait
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(main)
                main.wait_event(self._side_done)
                e1.record(main)
                prof.append(("wait_update", e0, e1))
            else:
                main.wait_event(self._side_done)
            self._side_done = None

    def training_step(self, inputs: Dict[str, Any], next_inputs: Optional[Dict[str, Any]] = None,
                      close_window: bool = False) -> torch.Tensor:
        """forward -> backward -> (all-reduce mean) -> clip -> Adafactor -> schedule.  With
        `overlap_comm` the tail runs on a side stream while the main stream already runs the frozen
        Whisper encoder of `next_inputs`."""
        model = self.model
        model.train()
        if self.args.gradient_accumulation_steps > 1:
            return self._accumulating_step(inputs, next_inputs, close_window)
        empty = self._is_empty_batch(inputs)
        if empty and self.world == 1:
            # HF loop on one device: zero loss, backward leaves every .grad None, Adafactor skips every parameter
            # (TF:optimization.py:1220) and so does torch AdamW (parameters, moments and its step count unchanged); the
            # scheduler and global_step still advance
            self.global_step += 1
            return self.compute_loss(model, inputs)
        prefetch = next_inputs is not None and not self._is_empty_batch(next_inputs)
        if prefetch and self._enc_stream is not None and not empty:
            # the frozen encoder of batch t+1 starts NOW on its own stream and runs beside this step's LLM forward / backward
            # (it reads nothing the optimizer writes)
            if self._side_done is not None and self.args.overlap_connector_backward:
                # the connector backward of step t-1 may still be reading the tapped-state buffer this prefetch is about to
                # overwrite (it runs on the side stream, which the encoder stream is otherwise not ordered behind)
                self._enc_stream.wait_event(self._side_done)
            model.prefetch_encoder(next_inputs["batch_features"], stream=self._enc_stream)
            prefetch = False
        self.wait_update()                                                    # connector weights of step t-1 are final
        loss = self.compute_loss(model, inputs)
        if empty:
            # data parallel: this rank MUST still enter the flat all-reduce and the optimizer step, or its peers block in the
            # collective forever and step counts diverge (under DDP the reference deadlocks here).  It contributes zeros: the
            # update is the mean over ranks with this rank's share empty.
            model.arena.grads.zero_()
            d_af = None
        elif self._side is not None and self.args.overlap_connector_backward:
            d_af = model.backward_llm()                                       # dX through the frozen LLM: main stream
        else:
            model.backward()
            d_af = None
        self.global_step += 1
        lr = linear_warmup_lr(self.global_step - 1, self.args.learning_rate, self.args.warmup_steps, self.total_steps)
        if self._side is None:
            self._reduce_and_update(lr)
            model._weights_dirty = False
        else:
            main = torch.cuda.current_stream(model.device)
            self._side.wait_stream(main)
            with torch.cuda.stream(self._side):
                if d_af is not None:
                    # the connector's backward (hundreds of small launches that leave most CUs idle) joins the tail on the side
                    # stream: the main stream goes straight on to the next batch's frozen Whisper forward, which reads nothing
                    # this half writes (its tapped states go to the OTHER encoder buffer)
                    d_af.record_stream(self._side)                            # allocated on the main stream, last read here
                    model.backward_connector(d_af)
                self._reduce_and_update(lr)
                ev = torch.cuda.Event()
                ev.record(self._side)
            self._side_done = ev
            model._weights_dirty = False
            if prefetch:                                                      # no encoder stream: overlap at least the optimizer tail
                model.prefetch_encoder(next_inputs["batch_features"])
        return loss

    def _accumulating_step(self, inputs: Dict[str, Any], next_inputs: Optional[Dict[str, Any]] = None,
                           close_window: bool = False) -> torch.Tensor:
        """`trainer.accumulate_grad_batches` > 1 (HF `gradient_accumulation_steps`, TF:trainer.py:1715-1813): every call is one
        MICRO-batch; its gradient arena is added into a second arena and the optimizer runs at every GA-th call — or earlier
        when `close_window` says the epoch's data ends here (HF's `remainder` window, TF:trainer.py:1715-1725, and
        `do_sync_step`, :1742).  The micro-batch gradients are SUMMED, not averaged: the reference's `forward(**kwargs)` makes
        `model_accepts_loss_kwargs` true (TF:trainer.py:500-505), so HF counts `num_items_in_batch`, hands it to
        `compute_loss` — which swallows it in **kwargs (desta_trainer.py:48) — and therefore does NOT divide the loss by the
        window length (TF:trainer.py:1952-1954; SURVEY hazard H8).  `global_step` counts optimizer steps.  An empty
        micro-batch contributes nothing.  No stream overlap on this path."""
        model, ga = self.model, self.args.gradient_accumulation_steps
        self.wait_update()
        loss = self.compute_loss(model, inputs)
        if self._acc is None:
            self._acc = torch.zeros_like(model.arena.grads)
        if not self._is_empty_batch(inputs):
            model.backward()
            if self._micro == 0:
                self._acc.copy_(model.arena.grads)
            else:
                from .. import _hip as H
                H.add_f32(self._acc, model.arena.grads)
        elif self._micro == 0:
            self._acc.zero_()
        self._micro += 1
        if self._micro < ga and not close_window:
            return loss
        self._micro = 0
        model.arena.grads.copy_(self._acc)
        self.global_step += 1
        lr = linear_warmup_lr(self.global_step - 1, self.args.learning_rate, self.args.warmup_steps, self.total_steps)
        self._reduce_and_update(lr)
        model._weights_dirty = False
        return loss

    def train(self, batches: Optional[Iterable[Dict[str, Any]]] = None, max_steps: Optional[int] = None,
              resume_from_checkpoint: Optional[str] = None):
        """`batches` given: ONE pass over that iterable of collated batches (tests, benchmarks).  Otherwise the HF loop shape
        (TF:trainer.py `_inner_training_loop`): epochs over `train_dataset` until `total_steps`, `checkpoint-<step>/` at every
        epoch end with save_strategy="epoch", and `resume_from_checkpoint` restores parameters / optimizer / schedule / step
        and skips the batches of the interrupted epoch that were already consumed (`steps_trained_in_current_epoch`)."""
        if resume_from_checkpoint:
            self.resume_from_checkpoint(resume_from_checkpoint)
        if batches is not None:
            losses = self._train_pass(iter(batches), max_steps)
        else:
            if self.train_dataset is None:
                raise ValueError("train() needs `batches` or train_dataset (+ data_collator)")
            total = self.total_steps if max_steps is None else min(self.total_steps, max_steps)
            spe = self.steps_per_epoch()
            losses = []
            epoch, skip = (self.global_step // spe, self.global_step % spe) if spe else (0, 0)
            while self.global_step < total:
                it = iter(self._epoch_batches(epoch))
                for _ in range(skip * self.args.gradient_accumulation_steps):        # micro-batches already consumed in this epoch
                    if next(it, None) is None:
                        break
                skip = 0
                before = self.global_step
                losses += self._train_pass(it, total)
                if self.global_step == before:
                    break                                                     # empty dataset
                epoch += 1
                if self.args.eval_strategy == "epoch" and self._can_evaluate():
                    self.evaluate()
                if self.args.save_strategy == "epoch" and (spe is None or self.global_step % spe == 0 or self.global_step >= total):
                    self.save_checkpoint(os.path.join(self.args.output_dir, f"checkpoint-{self.global_step}"))
        self.wait_update()
        self._sync()
        self.model.drop_prefetched()                                          # a prefetch for a batch that never ran is void
        self._flush_logs()
        return [float(x) for x in losses]

    def _sync(self) -> None:
        torch.cuda.synchronize(self.model.device)

    def _epoch_batches(self, epoch: int):
        ds = self.train_dataset
        if hasattr(ds, "batches"):                                            # streaming dataset that yields collated batches
            import inspect
            return ds.batches(epoch) if len(inspect.signature(ds.batches).parameters) >= 1 else ds.batches()
        if self.data_collator is None:
            raise ValueError("train() needs a data_collator for a map-style train_dataset")
        # torch DistributedSampler(shuffle, seed, drop_last=False) semantics: one permutation per epoch from seed + epoch, wrapped
        # to a multiple of the world size so EVERY rank draws the same number of batches (a rank that ran out early would leave
        # its peers in the gradient all-reduce), rank r takes every world-th sample.  (The HF / accelerate pipeline shards
        # BATCHES of a seeded RandomSampler instead: the sample -> rank assignment differs, the per-epoch coverage and
        # `steps_per_epoch` agree.)
        bs, n = self.args.per_device_train_batch_size, len(ds)
        if n == 0:
            return iter(())
        if self.args.shuffle:
            g = torch.Generator()
            g.manual_seed(self.args.seed + epoch)
            order = torch.randperm(n, generator=g).tolist()
        else:
            order = list(range(n))
        total = math.ceil(n / self.world) * self.world
        while len(order) < total:
            order += order[:total - len(order)]
        idx = order[self.rank:total:self.world]
        return self._collated(ds, [idx[s:s + bs] for s in range(0, len(idx), bs)])

    def _collated(self, ds, index_batches: List[List[int]]):
        """Collated batches of one epoch.  `dataloader_num_workers` > 0 and a collator with the host / device split
        (`BaseCollateFn.host_collate` / `.finish`): a torch DataLoader whose worker processes run the host half — WAVE decode,
        resampling, tokenisation, index arithmetic — `prefetch_factor` batches ahead, pinned by the loader's pin thread, while this
        process only applies the device half (H2D + log-mel kernel) and enqueues the step: the reference's
        `DataLoader(num_workers, pin_memory)` semantics (examples/train/train_desta.py:158-159, config/dataset/*.yaml).  Workers are
        FORKED and never touch the device.  Otherwise: inline on this thread."""
        coll, nw = self.data_collator, int(self.args.dataloader_num_workers)
        host, finish = getattr(coll, "host_collate", None), getattr(coll, "finish", None)
        if nw <= 0 or host is None or finish is None or not index_batches:
            return (coll([ds[i] for i in b]) for b in index_batches)
        from torch.utils.data import DataLoader, Dataset
        key = (id(ds), id(coll), nw, bool(self.args.dataloader_pin_memory))
        cached = getattr(self, "_loader", None)
        if cached is None or cached[0] != key:
            # ONE loader for the whole run: its worker processes are PERSISTENT and the batch sampler is an object whose contents are
            # replaced per epoch — a fresh DataLoader per epoch forks the workers again (measured: a 2.2-s stall at every epoch
            # boundary of `bench.py --data wav`, the parent holds 30 GB of page tables)
            class _Rows(Dataset):
                def __len__(self_inner):
                    return len(ds)

                def __getitem__(self_inner, i):
                    return ds[i]

            class _EpochIndexBatches:
                batches: List[List[int]] = []

                def __iter__(self_inner):
                    return iter(self_inner.batches)

                def __len__(self_inner):
                    return len(self_inner.batches)
            sampler = _EpochIndexBatches()
            dl = DataLoader(_Rows(), batch_sampler=sampler, collate_fn=host, num_workers=nw, pin_memory=bool(self.args.dataloader_pin_memory),
                            prefetch_factor=max(1, int(self.args.dataloader_prefetch_factor)), multiprocessing_context="fork", persistent_workers=True)
            cached = self._loader = (key, dl, sampler)
        _, dl, sampler = cached
        sampler.batches = index_batches
        return (finish(p) for p in dl)

    def _train_pass(self, it, max_steps: Optional[int]) -> List[torch.Tensor]:
        """One pass over an iterator of MICRO-batches (one epoch, or the caller's iterable).  Look-ahead and triggers follow
        the micro-batch position inside the accumulation window, not `global_step` alone: the batch after the current one is
        drawn unless the current one closes the window that reaches `max_steps`; a window is closed early only where the data
        ends (HF's shorter last window of an epoch); the step-driven evaluation fires once, right after an optimizer step."""
        ga = self.args.gradient_accumulation_steps
        losses: List[torch.Tensor] = []
        if max_steps is not None and self.global_step >= max_steps:
            return losses
        cur = next(it, None)
        while cur is not None:
            closes = self._micro == ga - 1                                    # this micro-batch completes its window
            final = max_steps is not None and closes and self.global_step + 1 >= max_steps
            nxt = None if final else next(it, None)
            before = self.global_step
            losses.append(self.training_step(cur, nxt, close_window=nxt is None))
            cur = nxt
            if (self.global_step != before and self.args.eval_strategy == "steps" and self.args.eval_steps
                    and self.global_step % self.args.eval_steps == 0 and self._can_evaluate()):
                self.evaluate()                                               # HF `_maybe_log_save_evaluate`: evaluate, then (epoch end) save
        return losses

    def _can_evaluate(self) -> bool:
        return self.eval_dataset is not None and self.data_collator is not None

    # -- evaluation (desta_trainer.py:104-189): eval loss / perplexity + generation through `_generate_step` ----------
    def evaluate(self, eval_batches: Optional[Iterable[Dict[str, Any]]] = None, metric_key_prefix: str = "eval",
                 generation_kwargs: Optional[Dict[str, Any]] = None) -> Dict[str, float]:
        """Eval-mode forward (no Q-Former dropout) for loss / ppl on every batch, then `_predict_step`.  The forward is
        `score_batch`, whose per-token argmax flags come from the same logits: `eval_token_accuracy` = target tokens that are
        the argmax / target tokens, summed over batches (and ranks) — teacher-forced next-token accuracy, no second pass.  Metrics keep the
        reference's names (`eval_loss`, `eval_ppl`); accuracy scoring needs the reference's text metrics and a tokenizer
        (`processing_class`) and is reported only when predictions could be decoded (`prediction_step_outputs`)."""
        dp = self.world > 1 and dist.is_available() and dist.is_initialized()
        sharded = False
        if eval_batches is None:
            if self.eval_dataset is None or self.data_collator is None:
                raise ValueError("evaluate() needs `eval_batches` or eval_dataset + data_collator")
            bs = self.args.per_device_eval_batch_size
            n = len(self.eval_dataset)
            # data parallel: rank r evaluates the batches r, r + world, ... of the unsharded batch list; losses and predictions
            # are combined below and only rank 0 writes the result files (HF shards the eval dataloader the same way and gathers)
            starts = list(range(0, n, bs))[self.rank::self.world] if dp else list(range(0, n, bs))
            sharded = dp
            eval_batches = (self.data_collator([self.eval_dataset[i] for i in range(s, min(s + bs, n))]) for s in starts)
        self.wait_update()
        was_training = self.model.training
        self.model.eval()
        losses: List[torch.Tensor] = []
        hits = torch.zeros(2, dtype=torch.float64, device=self.model.device)          # (target tokens that are the argmax, target tokens)
        self.prediction_step_outputs: List[Dict[str, Any]] = []
        try:
            for batch in eval_batches:
                if self._is_empty_batch(batch):
                    logging.warning("Skipping empty batch during evaluation")
                    continue
                fwd = {k: batch[k] for k in ("input_ids", "attention_mask", "batch_features", "batch_transcription_ids",
                                             "batch_start_positions", "labels") if k in batch}
                sc = self.model.score_batch(**fwd)
                losses.append(sc.loss.detach().clone())
                hits += torch.stack([sc.top1_match.sum(), sc.n_tokens.sum()]).double()
                if "context_input_ids" in batch:
                    self._predict_step(batch, generation_kwargs)
        finally:
            self.model.train(was_training)
        ls = torch.stack(losses).double() if losses else torch.zeros(0, dtype=torch.float64, device=self.model.device)
        agg = torch.stack([ls.sum(), torch.exp(ls).sum(), torch.tensor(float(len(losses)), dtype=torch.float64, device=self.model.device), hits[0], hits[1]])
        preds = self.prediction_step_outputs
        if sharded:
            if dist.get_backend() != "nccl":
                agg = agg.cpu()
            dist.all_reduce(agg, op=dist.ReduceOp.SUM)
            gathered: List[Any] = [None] * self.world
            dist.all_gather_object(gathered, preds)
            nb = max(len(g) for g in gathered)
            preds = [g[i] for i in range(nb) for g in gathered if i < len(g)]    # back to the unsharded batch order (per-batch rows stay together only for bs == 1; order is informational)
            self.prediction_step_outputs = preds
        cnt = float(agg[2])
        metrics = {f"{metric_key_prefix}_loss": float(agg[0]) / cnt if cnt else 0.0,
                   f"{metric_key_prefix}_ppl": float(agg[1]) / cnt if cnt else 0.0,
                   f"{metric_key_prefix}_token_accuracy": float(agg[3]) / float(agg[4]) if float(agg[4]) else 0.0}
        # desta_trainer.py:134-152: predictions JSONL + accuracy report under <exp_dir>/results/val, accuracy metrics
        exp_dir = self._cfg_get("exp_dir")
        decoded = bool(preds) and all("prediction" in r and "label" in r for r in preds)
        if exp_dir and (decoded or not preds):
            report: Dict[str, Any] = {}
            if self.rank == 0 or not sharded:
                spe = self.steps_per_epoch()
                epoch = (self.global_step / spe) if spe else 0.0
                ckpt = f"ep={epoch}-{self.global_step}"
                report = self._save_results(preds, os.path.join(exp_dir, "results", "val", f"val@{ckpt}.jsonl"), ckpt)
                report = {k: report.get(k) for k in ("accuracy_by_sample", "avg_accuracy_by_category", "categories_accuracy")}
            if sharded:
                box = [report]
                dist.broadcast_object_list(box, src=0)
                report = box[0]
            metrics[f"{metric_key_prefix}_accuracy"] = report.get("accuracy_by_sample") or 0
            metrics[f"{metric_key_prefix}_accuracy_by_category"] = report.get("avg_accuracy_by_category") or 0
            for category, acc in (report.get("categories_accuracy") or {}).items():
                metrics[f"{metric_key_prefix}_acc/{category}"] = acc
        self.log_history.append(dict(metrics))
        return metrics

    def _cfg_get(self, key: str, default=None):
        c = self.cfg
        if c is None:
            return default
        return c.get(key, default) if hasattr(c, "get") else getattr(c, key, default)

    def _save_results(self, results: List[Dict[str, Any]], filepath, ckpt: Optional[str] = None) -> Dict[str, Any]:
        """desta_trainer.py:191-251: `<dir>/preds/<name>.jsonl` (one row per prediction with `correct` and `index`; an existing
        file is never overwritten: `-1`, `-2`, ... — the reference's `lulutils.get_unique_filepath` is third-party and absent,
        its suffix rule is unpinned) and `<dir>/<name>-report.json` with per-sample / per-category accuracy."""
        import subprocess
        from collections import defaultdict
        from ..utils.metrics import ConsecutiveWordsAccuracyMetric
        metric = getattr(self, "metrics", None) or ConsecutiveWordsAccuracyMetric()
        filepath = str(filepath)
        d, name = os.path.join(os.path.dirname(filepath), "preds"), os.path.basename(filepath)
        os.makedirs(d, exist_ok=True)
        stem, ext = os.path.splitext(name)
        jsonl_path, k, f = os.path.join(d, name), 0, None
        while f is None:
            try:
                f = open(jsonl_path, "x")                                    # O_EXCL: two writers can never share a file
            except FileExistsError:
                k += 1
                jsonl_path = os.path.join(d, f"{stem}-{k}{ext}")
        by_cat = defaultdict(list)
        with f:
            for i, r in enumerate(results):
                r["correct"] = bool(metric(r["prediction"], r["label"]))
                r["index"] = i
                f.write(json.dumps(r, ensure_ascii=False) + "\n")
                by_cat[r.get("category", "all")].append(r["correct"])
        try:
            commit = subprocess.check_output("git rev-parse HEAD", shell=True, text=True, stderr=subprocess.DEVNULL).strip()
        except subprocess.SubprocessError:
            commit = None
        cfg = self.cfg
        if cfg is not None and not isinstance(cfg, dict) and hasattr(cfg, "items"):
            cfg = dict(cfg.items())
        exp_dir = (self.cfg.get("exp_dir") if hasattr(self.cfg, "get") else getattr(self.cfg, "exp_dir", None)) if self.cfg is not None else None
        report = {
            "metric": metric.metric_name,
            "preds_path": jsonl_path,
            "accuracy_by_sample": sum(r["correct"] for r in results) / (len(results) or 1),
            "avg_accuracy_by_category": (sum(sum(v) / len(v) for v in by_cat.values()) / len(by_cat)) if by_cat else 0,
            "categories_accuracy": {c: sum(v) / len(v) for c, v in by_cat.items()},
            "ckpt": str(ckpt),
            "results": [{k_: v for k_, v in r.items() if k_ not in {"context", "audio_context"}} for r in results],
            "exp_dir": exp_dir,
            "config": cfg if isinstance(cfg, dict) else None,
            "commit": commit,
            "name": "DeSTA2.5-Audio",
        }
        report_path = os.path.join(os.path.dirname(d), os.path.basename(jsonl_path).replace(".jsonl", "-report.json"))
        with open(report_path, "w") as f:
            json.dump(report, f, indent=2, ensure_ascii=False, default=str)
        logging.info(f"Report saved to {report_path}")
        return report

    def _predict_step(self, batch: Dict[str, Any], generation_kwargs: Optional[Dict[str, Any]] = None) -> torch.Tensor:
        """desta_trainer.py:160-189: generate from the context part of the batch; decode when a tokenizer is attached.
        generation_kwargs `logprobs` = n: every prediction row also carries `token_logprobs` (its tokens up to and including the
        first EOS, under the model's own distribution) and `avg_logprob`, their mean.  no_repeat_ngram_size, bad_words_ids,
        suppress_tokens, begin_suppress_tokens and min_new_tokens reach `_generate_step` when set (None: not passed), and so do
        typical_p, epsilon_cutoff and eta_cutoff."""
        cons = ("no_repeat_ngram_size", "bad_words_ids", "suppress_tokens", "begin_suppress_tokens", "min_new_tokens",
                "typical_p", "epsilon_cutoff", "eta_cutoff")
        gk = dict(temperature=0.7, top_p=0.9, max_new_tokens=128, do_sample=False, top_k=None, min_p=None, repetition_penalty=None,
                  logprobs=None, **{k: None for k in cons})
        cfg_gk = getattr(getattr(self.cfg, "model", None), "generation_kwargs", None) if self.cfg is not None else None
        for src in (cfg_gk, generation_kwargs):
            if src:
                gk.update({k: (src[k] if isinstance(src, dict) else getattr(src, k)) for k in gk if (k in src if isinstance(src, dict) else hasattr(src, k))})
        tok = self.processing_class
        eos_id = getattr(tok, "eos_token_id", None)
        pad_id = eos_id if eos_id is not None else 0

        def plain(v):                                                        # a YAML list arrives as a config node: the checks want lists
            return [plain(x) for x in v] if hasattr(v, "__iter__") and not isinstance(v, (str, bytes, dict)) else v
        ids = self.model._generate_step(batch, pad_token_id=pad_id, temperature=gk["temperature"], top_p=gk["top_p"],
                                        max_new_tokens=gk["max_new_tokens"], do_sample=gk["do_sample"],
                                        seed=self.global_step, top_k=gk["top_k"], min_p=gk["min_p"],
                                        repetition_penalty=gk["repetition_penalty"],
                                        **({} if gk["logprobs"] is None else {"logprobs": gk["logprobs"]}),
                                        **{k: plain(gk[k]) for k in cons if gk[k] is not None})
        extras = None
        if gk["logprobs"] is not None:
            ids, lp = ids
            eos = getattr(getattr(getattr(self.model, "config", None), "llm_config", None), "eos_token_id", eos_id)     # what `_generate_step` stopped on
            eos = [eos] if isinstance(eos, int) else list(eos or [])
            extras = []
            for row, vals in zip(ids.tolist(), lp.token_logprobs.tolist()):
                n = next((i + 1 for i, t in enumerate(row) if t in eos), len(row))
                extras.append({"avg_logprob": sum(vals[:n]) / max(n, 1), "token_logprobs": vals[:n]})
        metas = batch.get("metadata") or [{} for _ in range(ids.shape[0])]
        if extras is not None:
            metas = [{**m, **e} for m, e in zip(metas, extras)]
        if tok is not None:
            ctx = batch["context_input_ids"].clone()
            ctx[ctx == -100] = pad_id
            lab = batch["labels"].clone()
            lab[lab == -100] = pad_id
            contexts = tok.batch_decode(ctx, skip_special_tokens=False)
            labels = tok.batch_decode(lab, skip_special_tokens=True)
            preds = tok.batch_decode(ids, skip_special_tokens=True)
            for c, l, pr, m in zip(contexts, labels, preds, metas):
                self.prediction_step_outputs.append({**m, "context": c, "prediction": pr, "label": l})
        else:
            for row, m in zip(ids.cpu().tolist(), metas):
                self.prediction_step_outputs.append({**m, "prediction_ids": row})
        return ids

    # -- HF `checkpoint-<step>/` layout (TF:trainer.py `_save_checkpoint` / `_save_optimizer_and_scheduler` / `_save_rng_state`):
    #    model.safetensors (trainable-only) + config.json, optimizer.pt (Adafactor / AdamW state_dict wire format), scheduler.pt (LambdaLR
    #    state), trainer_state.json (TrainerState fields ONLY: `TrainerState.load_from_json` does cls(**json)), rng_state.pth
    #    (rng_state_<rank>.pth under data parallel), training_args.bin; this library's own resume data (forward counter and seed
    #    of the stateless dropout stream) lives in the sidecar desta_hip_state.json, which HF never opens.
    def _trainer_state(self) -> Dict[str, Any]:
        spe = self.steps_per_epoch()
        total = self._total_steps if self._total_steps is not None else (self.args.max_steps if self.args.max_steps > 0 else 0)
        return {
            "epoch": (self.global_step / spe) if spe else 0.0,
            "global_step": int(self.global_step),
            "max_steps": int(total),
            "logging_steps": int(self.args.logging_steps),
            "eval_steps": int(self.args.eval_steps) if self.args.eval_steps else 500,
            "save_steps": 500,
            "train_batch_size": int(self.args.per_device_train_batch_size),
            "num_train_epochs": int(math.ceil(self.args.num_train_epochs)),
            "num_input_tokens_seen": 0,
            "total_flos": 0.0,
            "log_history": self.log_history,
            "best_metric": None, "best_global_step": None, "best_model_checkpoint": None,
            "is_local_process_zero": True, "is_world_process_zero": True, "is_hyper_param_search": False,
            "trial_name": None, "trial_params": None, "stateful_callbacks": {},
        }

    def save_checkpoint(self, output_dir: str) -> None:
        import random
        from dataclasses import asdict
        import numpy as np
        from ..models.modeling_desta25 import reference_parameter_names
        self.wait_update()
        self._sync()
        os.makedirs(output_dir, exist_ok=True)
        # every rank: its own generator states (HF `_save_rng_state`; the sample order itself is a pure function of seed + epoch)
        rng = {"python": random.getstate(), "numpy": np.random.get_state(), "cpu": torch.random.get_rng_state(),
               "cuda": torch.cuda.get_rng_state(self.model.device) if torch.cuda.is_available() else None}
        if rng["cuda"] is None:
            del rng["cuda"]
        torch.save(rng, os.path.join(output_dir, "rng_state.pth" if self.world <= 1 else f"rng_state_{self.rank}.pth"))
        # the library's own resume data, PER RANK: the forward counter of the stateless dropout stream advances only on batches
        # with audio, so ranks that drew different `_empty_batch`es sit at different positions
        with open(os.path.join(output_dir, "desta_hip_state.json" if self.rank == 0 else f"desta_hip_state_{self.rank}.json"), "w") as f:
            json.dump({"forward_count": self.model._fwd_count, "dropout_seed": self.model.dropout_seed, "micro": self._micro,
                       "rank": self.rank, "world": self.world}, f, indent=1)
        if self.rank != 0:
            return
        self.model.save_pretrained(output_dir)
        lr = self.get_last_lr()
        torch.save(self.optimizer.hf_state_dict(reference_parameter_names(self.model.config), lr, self.args.weight_decay),
                   os.path.join(output_dir, "optimizer.pt"))
        torch.save({"base_lrs": [self.args.learning_rate] * 2, "last_epoch": self.global_step, "_step_count": self.global_step + 1,
                    "_get_lr_called_within_step": False, "_last_lr": [lr, lr], "lr_lambdas": [None, None]},
                   os.path.join(output_dir, "scheduler.pt"))
        torch.save(asdict(self.args), os.path.join(output_dir, "training_args.bin"))       # HF pickles its TrainingArguments; nothing reads it on resume
        self._flush_logs()
        with open(os.path.join(output_dir, "trainer_state.json"), "w") as f:
            f.write(json.dumps(self._trainer_state(), indent=2, sort_keys=True) + "\n")   # `TrainerState.save_to_json` format

    def resume_from_checkpoint(self, ckpt_dir: str) -> None:
        """Restore parameters, optimizer moments, schedule position, log history and the dropout stream position.  Reads
        checkpoints written by this trainer AND `checkpoint-<step>/` directories of the reference's HF Trainer (same
        model.safetensors keys, optimizer.pt / scheduler.pt wire formats, trainer_state.json)."""
        from safetensors.torch import load_file
        from ..models.modeling_desta25 import reference_parameter_names
        self.wait_update()
        self.model.load_state_dict(load_file(os.path.join(ckpt_dir, "model.safetensors")), strict=False)
        sd = torch.load(os.path.join(ckpt_dir, "optimizer.pt"), map_location="cpu", weights_only=True)
        self.optimizer.load_hf_state_dict(sd, reference_parameter_names(self.model.config))
        sched = torch.load(os.path.join(ckpt_dir, "scheduler.pt"), map_location="cpu", weights_only=True)
        self.global_step = int(sched["last_epoch"])
        st_path = os.path.join(ckpt_dir, "trainer_state.json")
        if os.path.isfile(st_path):
            with open(st_path) as f:
                st = json.load(f)
            self.global_step = int(st.get("global_step", self.global_step))
            self.log_history = list(st.get("log_history") or [])
            legacy = st.get("desta_hip") or {}                                 # round-2 files kept the sidecar data inside trainer_state.json
            self.model._fwd_count = int(legacy.get("forward_count", self.model._fwd_count))
        side = os.path.join(ckpt_dir, f"desta_hip_state_{self.rank}.json")
        if self.rank == 0 or not os.path.isfile(side):                        # rank 0's file also serves a run resumed on more ranks than it was saved on
            side = os.path.join(ckpt_dir, "desta_hip_state.json")
        if os.path.isfile(side):
            with open(side) as f:
                sc = json.load(f)
            self.model._fwd_count = int(sc.get("forward_count", self.model._fwd_count))
            if sc.get("dropout_seed") is not None and int(sc.get("world", self.world)) == self.world:
                self.model.dropout_seed = int(sc["dropout_seed"])
        # torch's generators (HF `_load_rng_state`): nothing on the hot path draws from them (dropout has its own counter RNG, the
        # sample order is a pure function of seed + epoch) — restored when the file holds plain tensors, for callers that do
        rp = os.path.join(ckpt_dir, "rng_state.pth" if self.world <= 1 else f"rng_state_{self.rank}.pth")
        if os.path.isfile(rp):
            try:
                rs = torch.load(rp, map_location="cpu", weights_only=True)
                if torch.is_tensor(rs.get("cpu")):
                    torch.random.set_rng_state(rs["cpu"])
                if torch.is_tensor(rs.get("cuda")) and torch.cuda.is_available():
                    torch.cuda.set_rng_state(rs["cuda"], self.model.device)
            except Exception:                                                 # noqa: BLE001 — python / numpy generator states need the unsafe loader: skipped
                pass
        self._micro = 0                                                       # checkpoints are written at window boundaries only
        self.model.refresh_weights()
        self.model._weights_dirty = False

    # -- checkpoint (trainable-only model.safetensors + optimizer state) --------------------------
    def save_model(self, output_dir: str) -> None:
        self.wait_update()
        if self.rank == 0:
            self.model.save_pretrained(output_dir)
