"""Exponential moving average of a model's weights on the MI355X (csrc/optim.hip: ym_ema_update, ym_adamw_ema).

The third staple of a YOLO training recipe next to augmentation and class-aware validation: the averaged copy,
not the raw last-step weights, is what gets validated, selected as best.pt and shipped.  The reference keeps no
average; `ModelEMA` follows the Ultralytics-style one (`ema = d * ema + (1 - d) * model` over the state dict after
every optimizer step, d ramping up as decay * (1 - exp(-updates / tau))), with the rule fixed as

    e = fma(omd, p - e, e)        fp32, omd = 1 - d formed in double and rounded once, p - e rounded once

`update()` is ONE launch over every fp32 entry of the state dict (parameters and BatchNorm running statistics).
With `FusedAdamW.attach_ema(ema)` the optimizer advances the counter itself, updates the EMA of every parameter
it steps inside its AdamW pass (the new value is still in a register there) and finishes with one launch over the
rest: the BatchNorm statistics and the parameters without a gradient.  `num_batches_tracked` is not averaged; it
is copied from the model whenever the EMA state is read.  The eval plan reads parameters and buffers at launch
time (yolomi/graph.py WeightStore.refresh, _eval_coeffs), so `.ema` validates through the graph-replayed inference
path as it is updated in place.  There is no CPU path: construction and state_dict work anywhere, update() needs
fp32 CUDA tensors.
"""
from __future__ import annotations

import copy
import math

import torch

from ._lib import EmaEntry, YolomiError, call, stream_ptr


def _copy_without_plans(model: torch.nn.Module) -> torch.nn.Module:
    """deepcopy of a module tree without what yolomi.graph caches on it (`_ym_plans` and friends hold activation
    buffers, pointer tables and captured graphs of the SOURCE model's tensors: the copy builds its own)."""
    held = []
    for m in model.modules():
        for k in [k for k in m.__dict__ if k.startswith("_ym_")]:
            held.append((m, k, m.__dict__.pop(k)))
    try:
        return copy.deepcopy(model)
    finally:
        for m, k, v in held:
            m.__dict__[k] = v


class ModelEMA:
    def __init__(self, model: torch.nn.Module, decay: float = 0.9999, tau: float = 2000, updates: int = 0):
        self.model = model
        self.ema = _copy_without_plans(model).eval()
        for p in self.ema.parameters():
            p.requires_grad_(False)
        self.decay, self.tau, self.updates = float(decay), float(tau), int(updates)
        self._tables = {}
        self._slots = None
        self._rest = None

    def decay_at(self, updates: int) -> float:
        """The decay of update number `updates` (>= 1): the Ultralytics warm-up ramp."""
        return self.decay * (1.0 - math.exp(-updates / self.tau))

    # ----------------------------------------------------------------- the launch
    def _float_slots(self):
        """Where every floating-point entry of the state dict lives, in its order: (the EMA module's parameter or
        buffer dict, the model's, the name in them, the state-dict key).  Found once (the two module trees are
        fixed); the tensors are looked up through the dicts at every update, so one that was replaced is seen."""
        if self._slots is None:
            src = dict(self.model.named_modules())
            slots = []
            for prefix, em in self.ema.named_modules():
                sm = src[prefix]
                for ed, sd in ((em._parameters, sm._parameters), (em._buffers, sm._buffers)):
                    for k, t in ed.items():
                        if t is not None and t.is_floating_point() and k not in em._non_persistent_buffers_set:
                            slots.append((ed, sd, k, f"{prefix}.{k}" if prefix else k))
            self._slots = slots
        return self._slots

    def _launch(self, slots, omd: float, tag):
        """ym_ema_update over `slots`; the device table is cached per tag and rebuilt (and the tensors checked)
        when any pointer changes."""
        if not slots:
            return
        key = tuple([p for ed, sd, k, _ in slots for p in (ed[k].data_ptr(), sd[k].data_ptr())])
        hit = self._tables.get(tag)
        if hit is None or hit[0] != key:
            arr = (EmaEntry * len(slots))()
            off = 0
            for ent, (ed, sd, k, name) in zip(arr, slots):
                e, s = ed[k], sd[k]
                if not (e.is_cuda and s.is_cuda and e.dtype == torch.float32 and s.dtype == torch.float32):
                    raise YolomiError("ModelEMA runs on the MI355X only: fp32 CUDA parameters and buffers "
                                      f"(got {name}: {s.dtype} on {s.device})")
                if not (e.is_contiguous() and s.is_contiguous()) or e.numel() != s.numel():
                    raise YolomiError(f"ModelEMA: dense contiguous tensors of one size required ({name})")
                ent.ema, ent.src, ent.offset, ent.n = e.data_ptr(), s.data_ptr(), off, e.numel()
                off += e.numel()
            dev = slots[0][0][slots[0][2]].device
            t = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
            hit = self._tables[tag] = (key, t, off, dev)
        call("ym_ema_update", hit[1].data_ptr(), len(slots), hit[2], omd, stream_ptr(hit[3]))

    def advance(self) -> float:
        """Count one update -> its 1 - decay (a Python double; the kernels round it to fp32 once)."""
        self.updates += 1
        return 1.0 - self.decay_at(self.updates)

    @torch.no_grad()
    def update(self):
        """One EMA update of every fp32 entry from the model's current state: one launch."""
        self._launch(self._float_slots(), 1.0 - self.decay_at(self.updates + 1), "all")       # (raises on a CPU model)
        self.updates += 1

    @torch.no_grad()
    def update_rest(self, stepped, omd: float):
        """The update of the entries an optimizer has not already averaged in its own pass; `stepped`: the tuple
        of the data pointers of the parameters it has (FusedAdamW.step).  Which entries are left is worked out
        again only when that tuple changes."""
        if self._rest is None or self._rest[0] != stepped:
            done = set(stepped)
            self._rest = (stepped, [sl for sl in self._float_slots() if sl[1][sl[2]].data_ptr() not in done])
        self._launch(self._rest[1], omd, "rest")

    def counterparts(self):
        """id(model parameter) -> the EMA module's parameter of the same name."""
        own = dict(self.ema.named_parameters())
        return {id(p): own[k] for k, p in self.model.named_parameters()}

    # ----------------------------------------------------------------- reading the state
    @torch.no_grad()
    def refresh(self):
        """The entries that are not averaged (num_batches_tracked) copied from the model: called where the EMA
        state is read (state_dict, validation), not per step."""
        src = self.model.state_dict()
        for k, e in self.ema.state_dict().items():
            if not e.is_floating_point():
                e.copy_(src[k])
        return self.ema

    def state_dict(self):
        return {"ema_state_dict": self.refresh().state_dict(), "ema_updates": self.updates}

    def load_state_dict(self, state):
        self.ema.load_state_dict(state["ema_state_dict"])
        self.updates = int(state["ema_updates"])

    @torch.no_grad()
    def seed(self, model: torch.nn.Module | None = None):
        """Restart the average from a model's current state (default: the tracked one) with updates = 0."""
        self.ema.load_state_dict((model or self.model).state_dict())
        self.updates = 0

    def sync_buffers(self, dp, src: int = 0):
        """Rank `src`'s EMA buffers everywhere (dp: a yolomi.dist.GradSync, or None).  The EMA parameters need
        no exchange: every rank applies the same all-reduced gradient to the same parameters, so they already
        agree bit for bit; the BatchNorm statistics follow each rank's own batches, as the model's do."""
        if dp is not None and dp.ctx.world > 1:
            from .dist import broadcast_buffers
            broadcast_buffers(self.ema, src)
