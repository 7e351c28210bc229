"""Optimizers.  ``build_optimizer`` mirrors src/dprt/training/optimizer.py:6-7 (``getattr(torch.optim,
name)``); for AdamW on CUDA it returns ``FusedAdamW``: the same update rule as torch.optim.AdamW
(lr, betas=(0.9,0.999), eps=1e-8, weight_decay=1e-2, no amsgrad) executed by ONE HIP launch over all
parameter tensors (dpft_adamw_f32), with the moments in two flat fp32 buffers (per-parameter state kept)."""
from __future__ import annotations

import numpy as np
import torch

from dpft_amd.hip.lib import lib, note_weights_changed, ptr, stream

CHUNK = 16384


def ema_decay_ok(decay) -> bool:
    """A usable EMA decay: a real number (not a bool) that lies in [0, 1) AFTER rounding to fp32, the form in which it crosses
    the C boundary (0.99999999 rounds to 1.0 and is refused).  Never raises: an int too large for a float is simply not usable."""
    if isinstance(decay, bool) or not isinstance(decay, (int, float)):
        return False
    try:
        d = float(decay)
    except OverflowError:
        return False
    return 0.0 <= d < 1.0 and float(np.float32(d)) < 1.0


class FusedAdamW(torch.optim.Optimizer):
    """Drop-in for ``torch.optim.AdamW`` (no amsgrad / maximize / capturable).  The moments of a parameter group live in
    two flat fp32 buffers; ``self.state[p]`` holds views into them, so ``state_dict()`` / ``load_state_dict()`` round-trip
    in torch's format.  Fast path: persistent gradient buffers (the DP reducer's buckets) - the pointer table is built
    once.  With a plain ``zero_grad(set_to_none=True)`` loop the table is re-pointed whenever a ``.grad`` moves; the
    moments and step counts are keyed by parameter and survive that.  ``grad is None`` = the parameter sits the step out
    (its own step count does not advance, exactly like torch)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        super().__init__(list(params), dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self._tables = None
        self._step = 0                 # launches so far; a tensor's own count is _step - skipped[t]
        self._restore = False          # self.state was replaced by load_state_dict: re-seed the flat buffers from it
        # Segments (round 4): the DP reducer's buckets.  A bucket whose gradients are final (all produced, all-reduced) can
        # be stepped at once, on the stream that finished it, while the backward goes on elsewhere -- step_segment();
        # step() then only launches what is left.  Rows of the chunk table are ordered by segment for that.
        self._segments = None          # list of lists of parameters (a parameter not listed belongs to the trailing segment)
        self._round_open = False       # a step_segment() of the current step has already advanced _step
        self._done = set()             # (table index, segment index) launched in the current step
        # Clipping by global L2 norm (set_clip): off unless asked for.  _partials = one double per chunk-table row of every
        # group, _clip_record = the 16 bytes {norm, coef, nonfinite, nonfinite_total} the norm launches leave for the AdamW launch.
        self._clip = None              # (max_norm, nonfinite mode 0 | 1)
        self._partials = None
        self._clip_record = None
        # EMA of the weights (set_ema): off unless asked for.  A third flat buffer per group, laid out like the moments.
        self._ema = None               # (decay, warmup 0 | 1)

    NONFINITE_MODES = {"propagate": 0, "skip": 1}

    def set_clip(self, max_norm, nonfinite: str = "propagate"):
        """Clip the gradients by their global L2 norm inside step(), on the device: ``torch.nn.utils.clip_grad_norm_(params,
        max_norm)`` (norm_type 2, error_if_nonfinite=False) followed by the AdamW update, without a host read-back and without
        touching the gradients -- the update uses ``g * coef`` in registers, ``.grad`` KEEPS THE UNCLIPPED gradient.  The norm
        covers the parameters that take part in the step (a gradient this step, active, gate open or not).  ``max_norm=None``
        switches clipping off.  ``nonfinite``: what a NaN / infinite norm does -- "propagate" (torch: the coefficient is NaN or 0
        and the parameters follow) or "skip" (the step is dropped exactly like a closed gate: nothing moves, the per-parameter
        step counts do not advance, nonfinite_steps() counts it)."""
        assert not self._round_open, "FusedAdamW.set_clip between step_segment() and step()"
        if max_norm is None:
            self._clip = None
            return
        if nonfinite not in self.NONFINITE_MODES:
            raise ValueError(f"nonfinite must be 'propagate' or 'skip', not {nonfinite!r}")
        if isinstance(max_norm, bool) or not isinstance(max_norm, (int, float)) or not (0.0 < float(max_norm) < float("inf")):
            raise ValueError(f"max_norm must be a finite positive number, not {max_norm!r}")
        self._clip = (float(max_norm), self.NONFINITE_MODES[nonfinite])
        if self._clip_record is None:      # allocated once: nonfinite_total lives in it
            dev = next(p for g in self.param_groups for p in g["params"]).device
            self._clip_record = torch.zeros(4, dtype=torch.int32, device=dev)

    def set_ema(self, decay, warmup: bool = False):
        """Keep an exponential moving average of the weights inside step(): ``ema.lerp_(p, 1 - decay)`` on every element the
        launch updates (the rule of ``torch.optim.swa_utils.get_ema_multi_avg_fn``), in a flat fp32 buffer per group laid out
        like the moments and seeded with the current parameter values.  A tensor that sits a step out (no gradient, closed
        gate, a step dropped by clipping's "skip" mode) keeps its average.  ``warmup``: the decay of a tensor's n-th own step is
        ``min(decay, (1 + n) / (10 + n))``.  ``self.state[p]["ema"]`` views the buffer, so state_dict() / load_state_dict()
        carry it.  ``decay=None`` switches the EMA off and drops the buffers."""
        assert not self._round_open, "FusedAdamW.set_ema between step_segment() and step()"
        if decay is None:
            self._ema = None
            for t in self._tables or []:
                for k in ("ema", "swap", "n_swap"):
                    t.pop(k, None)
            for st in self.state.values():
                st.pop("ema", None)
            return
        if not ema_decay_ok(decay):
            raise ValueError(f"decay must be a number in [0, 1) (as a float32), not {decay!r}")
        if not isinstance(warmup, (bool, np.bool_)):
            raise ValueError(f"warmup must be a bool, not {warmup!r}")
        self._ema = (float(decay), int(bool(warmup)))
        if self._tables is not None and not self._restore:
            for t in self._tables:
                if "ema" not in t:
                    self._seed_ema(t)

    def _seed_ema(self, t):
        """Allocate the table's flat ``ema`` buffer next to m / v, seed it from the parameters (or from a loaded / carried-over
        ``state[p]["ema"]``), and build the table swap_ema() launches over: every trainable parameter, with or without a
        gradient row at the moment."""
        ema = torch.empty_like(t["m"])
        rows, off = [], 0
        with torch.no_grad():
            for p in t["params"]:
                view = self._flat_view(ema, off, p)
                st = self.state[p]
                src = st["ema"] if "ema" in st else p
                view.copy_(src.detach())
                st["ema"] = view
                for c0 in range(0, p.numel(), CHUNK):
                    rows.append((p.data_ptr() + 4 * c0, ema.data_ptr() + 4 * (off + c0), min(CHUNK, p.numel() - c0), 0))
                off += p.numel()
        arr = np.zeros(len(rows), dtype=np.dtype([("a", "<u8"), ("b", "<u8"), ("n", "<i4"), ("pad", "<i4")]))
        for i, r in enumerate(rows):
            arr[i] = r
        t["ema"] = ema
        t["swap"] = torch.from_numpy(arr.view(np.uint8).copy()).to(ema.device)
        t["n_swap"] = len(rows)

    def ema_parameters(self):
        """The EMA of every trainable parameter, in parameter order: views into the flat buffers (shape and physical element
        order of the parameter).  Needs set_ema() and built tables (a step(), or build_tables())."""
        assert self._ema is not None, "ema_parameters() needs set_ema()"
        self.build_tables()
        return [self.state[p]["ema"] for t in self._tables for p in t["params"]]

    def build_tables(self):
        """Build the chunk tables (and the EMA buffers) now instead of at the first step(), if they are missing or stale."""
        if self._restore or self._tables is None:
            assert not self._round_open
            self._build()

    @torch.no_grad()
    def swap_ema(self):
        """Exchange the weights and their EMA in place, one dpft_swap_f32 launch per group: afterwards the parameters hold the
        former EMA bits and the EMA buffer the former parameter bits; a second call restores both.  Covers every trainable
        parameter of the group, also one that has no gradient at the moment."""
        assert self._ema is not None, "swap_ema() needs set_ema()"
        assert not self._round_open, "FusedAdamW.swap_ema between step_segment() and step()"
        self.build_tables()
        for t in self._tables:
            if any(p.data_ptr() != a for p, (a, _) in zip(t["params"], t["ptrs"])):
                self._build()                                   # a parameter's storage moved: re-point the tables
                break
        for t in self._tables:
            lib.call("dpft_swap_f32", ptr(t["swap"]), t["n_swap"], stream())
        note_weights_changed()

    def last_grad_norm(self):
        """The global gradient norm of the last clipped step BEFORE clipping (what clip_grad_norm_ returns): a device scalar
        that views the clip record -- no synchronisation, the next step overwrites it.  None when clipping was never on."""
        return None if self._clip_record is None else self._clip_record.view(torch.float32)[0]

    def nonfinite_steps(self) -> int:
        """Steps whose gradient norm was not finite in "skip" mode.  Reads the counter back (synchronises).  The norm launches
        do not see the `loss > 0` gate, so a step that the gate closed anyway is counted too when its gradients were not finite
        (a NaN loss does both: it closes the gate and makes the gradients NaN); last_grad_norm() of such a step is NaN as well."""
        return 0 if self._clip_record is None else int(self._clip_record[3])

    def grad_sqnorms(self):
        """Per-tensor squared gradient norms of the last clipped step, fp64, one device tensor per parameter group with one
        entry per trainable parameter (0 for a tensor that sat the step out).  Computed on demand from the per-row partial
        sums; not on the step path."""
        assert self._partials is not None and self._tables is not None, "grad_sqnorms() needs a step() with clipping on"
        out = []
        for t in self._tables:
            idx = torch.from_numpy(t["row_tensor"]).to(self._partials.device)
            part = self._partials[t["part_off"]:t["part_off"] + t["n_chunks"]]
            out.append(torch.zeros(len(t["params"]), dtype=torch.float64, device=part.device).index_add_(0, idx, part))
        return out

    def _size_partials(self):
        """One double per row of every group's table; each table owns the range starting at its part_off."""
        total = 0
        for t in self._tables:
            t["part_off"] = total
            total += t["n_chunks"]
        self._partials = torch.zeros(total, dtype=torch.float64, device=self._tables[0]["chunks"].device)

    def attach_segments(self, param_lists):
        """Declare the segments (lists of parameters, e.g. GradBucketReducer buckets) step_segment() may be called with."""
        self._segments = [list(ps) for ps in param_lists]
        self._tables = None            # rebuilt (row order) at the next step

    @staticmethod
    def _layout(t: torch.Tensor):
        """Set of dense physical element orders a tensor has: 'plain' (row-major) and/or 'khwc'."""
        out = set()
        if t.is_contiguous():
            out.add("plain")
        if t.dim() == 4 and t.permute(0, 2, 3, 1).is_contiguous():
            out.add("khwc")
        return out

    @staticmethod
    def _ptrs(ps):
        return [(p.data_ptr(), None if p.grad is None else p.grad.data_ptr()) for p in ps]

    @staticmethod
    def _flat_view(flat, off, p):
        """View of ``flat[off : off + numel]`` with p's shape AND physical element order."""
        v = flat[off:off + p.numel()]
        if p.dim() == 4 and not p.is_contiguous():                    # khwc
            o, i, kh, kw = p.shape
            return v.view(o, kh, kw, i).permute(0, 3, 1, 2)
        return v.view(p.shape)

    def _build(self):
        """(Re)build the chunk tables.  Moments: first build -> zeros (or the loaded state); later builds keep the flat
        buffers and only refresh the parameter / gradient pointers."""
        old = self._tables
        if self._restore:
            steps = [float(st["step"]) for st in self.state.values() if "step" in st]
            self._step = int(max(steps)) if steps else 0
        tables = []
        if old is not None and not self._restore:
            # a group whose set of trainable parameters changed gets new flat buffers: the per-parameter step counts live
            # only in the old tables' device-side `skipped` counters (state["step"] is written by state_dict() alone), so
            # they are read back here -- otherwise a carried-over parameter would restart its bias correction at 0
            for gi, group in enumerate(self.param_groups):
                ps = [p for p in group["params"] if p.requires_grad]
                if gi < len(old) and [id(p) for p in old[gi]["params"]] != [id(p) for p in ps]:
                    for p, sk in zip(old[gi]["params"], old[gi]["skipped"].tolist()):
                        if p in self.state:
                            self.state[p]["step"] = float(self._step - int(sk))
        for gi, group in enumerate(self.param_groups):
            ps = [p for p in group["params"] if p.requires_grad]
            dev = ps[0].device
            keep = old is not None and not self._restore and gi < len(old) and \
                [id(p) for p in old[gi]["params"]] == [id(p) for p in ps]
            if keep:
                m, v, skipped = old[gi]["m"], old[gi]["v"], old[gi]["skipped"]
                carried = {k: old[gi][k] for k in ("ema", "swap", "n_swap") if k in old[gi]}
            else:
                total = sum(p.numel() for p in ps)
                m = torch.zeros(total, dtype=torch.float32, device=dev)
                v = torch.zeros(total, dtype=torch.float32, device=dev)
                skip_host = [0] * len(ps)
            rows, off = [], 0
            seg_of = {}
            if self._segments is not None:
                for si, sp in enumerate(self._segments):
                    for q in sp:
                        seg_of[id(q)] = si
            n_seg = (len(self._segments) if self._segments is not None else 0) + 1      # + the trailing segment
            seg_rows = [[] for _ in range(n_seg)]
            seg_tensors = [[] for _ in range(n_seg)]
            for ti, p in enumerate(ps):
                rows = seg_rows[seg_of.get(id(p), n_seg - 1)]
                seg_tensors[seg_of.get(id(p), n_seg - 1)].append(ti)
                mv, vv = self._flat_view(m, off, p), self._flat_view(v, off, p)
                if not keep:
                    st = self.state.get(p, {})
                    if "exp_avg" in st:                                # loaded / carried-over state
                        mv.copy_(st["exp_avg"])
                        vv.copy_(st["exp_avg_sq"])
                        skip_host[ti] = self._step - int(float(st.get("step", 0)))
                    else:
                        skip_host[ti] = self._step                      # joins now: its own count starts at 0
                    self.state[p] = {"exp_avg": mv, "exp_avg_sq": vv}
                    if "ema" in st:                                    # re-homed in the group's new buffer by _seed_ema
                        self.state[p]["ema"] = st["ema"]
                rows.append((0, 0, 0, 0, 0, ti))                        # marker row (advances skipped[t] when inactive)
                if p.grad is not None:
                    assert p.grad.dtype == torch.float32 and (self._layout(p) & self._layout(p.grad)), \
                        "FusedAdamW expects dense fp32 gradients laid out like their parameters"
                    pp, gp = p.data_ptr(), p.grad.data_ptr()
                    for c0 in range(0, p.numel(), CHUNK):
                        n = min(CHUNK, p.numel() - c0)
                        rows.append((pp + 4 * c0, gp + 4 * c0, m.data_ptr() + 4 * (off + c0),
                                     v.data_ptr() + 4 * (off + c0), n, ti))
                off += p.numel()
            seg_range, rows = [], []
            for sr in seg_rows:                                         # rows of a segment are contiguous in the table
                seg_range.append((len(rows), len(sr)))
                rows += sr
            if not keep:
                skipped = torch.tensor(skip_host, dtype=torch.int32).to(dev)
            arr = np.zeros(len(rows), dtype=np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"),
                                                      ("n", "<i4"), ("t", "<i4")]))
            for i, r in enumerate(rows):
                arr[i] = r
            chunks = torch.from_numpy(arr.view(np.uint8).copy()).to(dev)
            active = torch.ones(len(ps), dtype=torch.int32, device=dev)
            tables.append(dict(params=ps, ptrs=self._ptrs(ps), m=m, v=v, skipped=skipped, chunks=chunks,
                               n_chunks=len(rows), active=active, active_host=None, seg_range=seg_range,
                               seg_tensors=seg_tensors, row_tensor=arr["t"].astype(np.int64)))
            if keep:
                tables[-1].update(carried)
            if self._ema is not None and (not keep or "ema" not in carried or
                                          [p.data_ptr() for p in ps] != [a for a, _ in old[gi]["ptrs"]]):
                self._seed_ema(tables[-1])
            elif self._ema is None:
                for p in ps:
                    self.state[p].pop("ema", None)
        self._tables = tables
        self._restore = False
        self._partials = None
        if self._clip is not None:
            self._size_partials()

    @torch.no_grad()
    def launch_tables(self):
        """The AdamW launches of step() alone, one per group over the tables as they stand: no pointer check, no refresh of the
        `active` flags, no norm launches, no gate.  It IS an update (the step count advances, parameters, moments and the EMA
        move, with whatever the gradient buffers hold).  For measurement (tools/ema_cost.py): needs a step() before it."""
        assert self._tables is not None and not self._restore and not self._round_open, "launch_tables() needs a step() first"
        self._step += 1
        for group, t in zip(self.param_groups, self._tables):
            self._launch(group, t, 0, t["n_chunks"])
        note_weights_changed()

    def set_gate(self, loss: "torch.Tensor" = None):
        """Device-side `if loss > 0` (trainer.py:131) for the NEXT step(): a scalar tensor that stays on the device; the launch
        updates nothing when it is not positive.  Consumed by step()."""
        self._gate = loss

    def set_active(self, active_ids):
        """ids of parameters that received a gradient this step (others are skipped like ``grad is None``)."""
        self._active_ids = active_ids

    CHUNK_BYTES = 40

    def _launch(self, group, t, first: int, count: int):
        if count <= 0:
            return
        b1, b2 = group["betas"]
        import ctypes as C
        args = (C.c_void_p(t["chunks"].data_ptr() + first * self.CHUNK_BYTES), count, ptr(t["active"]), ptr(t["skipped"]),
                float(group["lr"]), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]),
                self._step, ptr(getattr(self, "_gate", None)))
        if self._ema is not None:
            lib.call("dpft_adamw_ema_f32", *args, ptr(self._clip_record) if self._clip is not None else None,
                     ptr(t["m"]), ptr(t["ema"]), self._ema[0], self._ema[1], stream())
        elif self._clip is not None:
            lib.call("dpft_adamw_clip_f32", *args, ptr(self._clip_record), stream())
        else:
            lib.call("dpft_adamw_f32", *args, stream())

    def _launch_norm(self):
        """The two norm launches of a clipped step: the sum of squares of every group's table into its range of the partials,
        then one workgroup that adds the partials up and writes the clip record."""
        import ctypes as C
        if self._partials is None:
            self._size_partials()
        for t in self._tables:
            lib.call("dpft_grad_sqnorm_f32", ptr(t["chunks"]), t["n_chunks"], ptr(t["active"]),
                     C.c_void_p(self._partials.data_ptr() + 8 * t["part_off"]), stream())
        lib.call("dpft_grad_clip_coef_f32", ptr(self._partials), self._partials.numel(), self._clip[0], self._clip[1],
                 ptr(self._clip_record), stream())

    @torch.no_grad()
    def step_segment(self, si: int) -> bool:
        """Update the parameters of segment ``si`` NOW, on the current stream (their gradients are final there).  Returns
        False -- and leaves the segment to step() -- when the tables are stale or a tensor of the segment sat the previous
        step out (its `active` flag on the device would have to change first).  The step count advances once per step."""
        if self._segments is None or self._restore or self._tables is None:
            return False
        if self._clip is not None:
            return False      # the coefficient needs the norm over ALL buckets: no bucket can be stepped before step()
        if getattr(self, "gate_required", False) and getattr(self, "_gate", None) is None:
            return False      # the step's `loss > 0` decision is taken on the device: never launch ahead of its gate
        if any(self._ptrs(t["params"]) != t["ptrs"] for t in self._tables):
            return False
        todo = []
        for gi, (group, t) in enumerate(zip(self.param_groups, self._tables)):
            first, count = t["seg_range"][si]
            if count == 0 or (gi, si) in self._done:
                continue
            host = t["active_host"]
            if host is None or any(host[ti] != 1 for ti in t["seg_tensors"][si]):
                return False
            todo.append((gi, group, t, first, count))
        if not self._round_open:
            self._step += 1
            self._round_open = True
        for gi, group, t, first, count in todo:
            self._launch(group, t, first, count)
            self._done.add((gi, si))
        return True

    @torch.no_grad()
    def step(self, closure=None):
        if self._restore or self._tables is None or any(self._ptrs(t["params"]) != t["ptrs"] for t in self._tables):
            assert not self._round_open, "FusedAdamW: gradients moved between step_segment() and step()"
            self._build()
        if not self._round_open:
            self._step += 1
        ids = getattr(self, "_active_ids", None)
        for gi, (group, t) in enumerate(zip(self.param_groups, self._tables)):
            host = [int(p.grad is not None and (ids is None or id(p) in ids)) for p in t["params"]]
            if host != t["active_host"]:
                # (tensors of segments already stepped in this round were all active, before and now: their flags do not move)
                t["active"].copy_(torch.tensor(host, dtype=torch.int32))
                t["active_host"] = host
        if self._clip is not None:
            self._launch_norm()
        for gi, (group, t) in enumerate(zip(self.param_groups, self._tables)):
            if not any(g == gi for g, _ in self._done):
                self._launch(group, t, 0, t["n_chunks"])                # nothing stepped early: the one launch of before
            else:
                for si, (first, count) in enumerate(t["seg_range"]):
                    if (gi, si) not in self._done:
                        self._launch(group, t, first, count)
        self._round_open = False
        self._done.clear()
        self._gate = None
        note_weights_changed()                             # in-place through raw pointers: no _version bump
        return None

    def state_dict(self):
        """torch's format: per parameter ``step`` (its own count), ``exp_avg``, ``exp_avg_sq``."""
        for t in self._tables or []:
            skipped = t["skipped"].cpu().tolist()
            for p, sk in zip(t["params"], skipped):
                self.state[p]["step"] = torch.tensor(float(self._step - sk))
        return super().state_dict()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._restore = True


def build_optimizer(name: str, params, device=None, **kwargs):
    if name == "AdamW" and device is not None and torch.device(device).type == "cuda" and not kwargs.get("amsgrad"):
        return FusedAdamW(params, **kwargs)
    return getattr(torch.optim, name)(params, **kwargs)
