"""Fused clip + SGD-Nesterov and clip + Adam / AdamW on flat buffers, the reference's PolyLR schedule and cosine annealing.

Replaces `torch.nn.utils.clip_grad_norm_(params, 12)` + `torch.optim.SGD(lr 1e-2, wd 3e-5, momentum .99,
nesterov).step()` (nnUNet/nnunetv2/training/nnUNetTrainer/nnUNetTrainer.py:473-477, :918-924),
PolyLRScheduler (nnUNet/nnunetv2/training/lr_scheduler/polylr.py:4-20), the `torch.optim.AdamW(amsgrad=True)` /
`torch.optim.Adam` of variants/optimizer/nnUNetTrainerAdam.py and the `CosineAnnealingLR` of
variants/lr_schedule/nnUNetTrainerCosAnneal.py.
"""
import ctypes
import math

import torch

from . import ops
from ._lib import call, query


class FlatParams:
    """Re-homes the parameters of a module into ONE flat fp32 buffer (and their .grad into another), 16-byte
    aligned per tensor, so that the optimizer, the gradient-norm and the DDP buckets are single contiguous ranges.
    Parameter objects, names and state_dict keys are untouched (p.data becomes a view)."""

    ALIGN = 4  # floats

    def __init__(self, params):
        # `params`: parameters, or (name, parameter) pairs -- the names go into layout() so that a saved optimizer state
        # can be matched to the parameters of a differently ordered buffer
        pairs = [q if isinstance(q, (tuple, list)) else (None, q) for q in params]
        pairs = [(n, p) for n, p in pairs if p.requires_grad]
        # de-duplicate shared parameters (decoder.encoder.* aliases) preserving order
        seen, uniq = set(), []
        for n, p in pairs:
            if id(p) not in seen:
                seen.add(id(p))
                uniq.append((n, p))
        self.names = [n for n, _ in uniq]
        self.params = [p for _, p in uniq]
        dev = self.params[0].device
        self.offsets, off = [], 0
        for p in self.params:
            self.offsets.append(off)
            off += (p.numel() + self.ALIGN - 1) // self.ALIGN * self.ALIGN
        self.numel = off
        self.flat = torch.zeros(off, dtype=torch.float32, device=dev)
        # packed-weight cache (ops.py): epoch of THIS buffer (bumped by the optimizer that updates it through a raw pointer),
        # and -- when a trainer replays its step as a hipGraph -- bf16 packs kept in one persistent buffer owned by this
        # object and rewritten in place, with a generation counter guarding autograd graphs saved across the rewrite
        self.flat._mvd_epoch = [0]
        self.pack16_inplace = False
        self.pack16_gen = [0]
        self.flat._mvd_pack16_gen = self.pack16_gen
        self._pack16_buf = None
        self.grad = torch.zeros(off, dtype=torch.float32, device=dev)
        # direct gradient sink (ops.py): the HIP backward kernels write dW / dbias / dgamma / dbeta straight into this
        # buffer instead of returning fresh tensors that autograd would add into p.grad with one small torch kernel per
        # parameter (~1 ms per step).  A parameter can be taken once per step (zero_grad() starts a new step); a second
        # contribution in the same step goes through autograd's accumulation as before.
        self.step_id = 0
        self._written = [-1] * len(self.params)
        self.listeners = []   # callables(index): "the gradient of parameter index is complete" (BucketedGradReducer)
        with torch.no_grad():
            for p, o in zip(self.params, self.offsets):
                view = self.flat[o:o + p.numel()].view(p.shape)
                view.copy_(p.data)
                p.data = view
                p._mvd_flat = self.flat   # ops' packed-weight cache also watches the flat buffer's version counter
        self.attach_grads()

    def layout(self):
        """What a flat state buffer (the momentum) has to agree on to be loaded here: per parameter (name or None,
        shape, offset), in buffer order."""
        return [(n, tuple(p.shape), o) for n, p, o in zip(self.names, self.params, self.offsets)]

    def invalidate_packs(self):
        """Call after writing parameter memory behind torch's back (`p.data.copy_()`, a raw-pointer kernel): the
        packed weight copies the conv kernels read are rebuilt at the next forward."""
        ops.invalidate_packs()

    def attach_grads(self):
        for i, (p, o) in enumerate(zip(self.params, self.offsets)):
            p.grad = self.grad[o:o + p.numel()].view(p.shape)
            p._mvd_take_grad = self._make_take(i)
            p._mvd_grad_done = self._make_done(i)

    def _make_take(self, i):
        def take():
            if self._written[i] == self.step_id:
                return None
            self._written[i] = self.step_id
            return self.params[i].grad
        return take

    def _make_done(self, i):
        def done():
            for fn in self.listeners:
                fn(i)
        return done

    def zero_grad(self):
        self.grad.zero_()
        self.step_id += 1
        self.attach_grads()


def _place_flat_state(src, theirs, fp, what):
    """A flat optimizer-state buffer `src` saved under the layout `theirs` (FlatParams.layout(), or None: written before
    the signature existed), as a tensor laid out like `fp.flat`.  Same layout (or none): `src` itself when its size matches.
    Another layout with unique names on both sides that cover the same parameters (same names and shapes, another
    order): every parameter's slice moved to its place here.  Anything else raises ValueError; nothing is written."""
    mine = fp.layout()
    theirs = [(n, tuple(shape), int(o)) for n, shape, o in theirs] if theirs is not None else None
    if theirs is None or theirs == mine:
        if src.numel() != fp.numel:
            raise ValueError(f"optimizer state: {what} buffer of {src.numel()} elements, this parameter layout "
                             f"has {fp.numel}")
        return src
    by_name = {n: (shape, o) for n, shape, o in theirs}
    names = [n for n, _, _ in mine]
    if None in by_name or None in names or len(by_name) != len(theirs) or len(set(names)) != len(names) or \
            set(by_name) != set(names) or any(by_name[n][0] != shape for n, shape, _ in mine):
        raise ValueError(f"optimizer state: parameter layout mismatch -- the {what} buffer was saved under another "
                         "parameter order or other shapes, and the two layouts cannot be matched by name "
                         f"(saved: {[(n, s) for n, s, _ in theirs][:4]}..., here: {[(n, s) for n, s, _ in mine][:4]}...)")
    need = max(o + math.prod(shape) for _n, shape, o in theirs)
    if src.numel() < need:
        raise ValueError(f"optimizer state: parameter layout mismatch -- the saved layout covers {need} elements, "
                         f"the saved {what} buffer has {src.numel()}")
    src = src.to(fp.flat.device)
    new = torch.zeros(fp.numel, dtype=src.dtype, device=fp.flat.device)
    for n, shape, o in mine:
        k, so = math.prod(shape), by_name[n][1]
        new[o:o + k] = src[so:so + k]
    return new


class FusedSGDNesterov:
    """Optimizer-like object (zero_grad / step / param_groups / state_dict) driving mvd_grad_sumsq +
    mvd_sgd_nesterov_step.  The clip coefficient is computed on the device: no host sync in the step."""

    def __init__(self, params, lr=1e-2, weight_decay=3e-5, momentum=0.99, nesterov=True, max_grad_norm=12.0):
        if not nesterov:
            raise NotImplementedError("the reference trains with nesterov=True")
        self.fp = params if isinstance(params, FlatParams) else FlatParams(list(params))
        self.param_groups = [{'lr': lr, 'weight_decay': weight_decay, 'momentum': momentum, 'nesterov': True,
                              'params': self.fp.params}]
        self.max_grad_norm = max_grad_norm
        dev = self.fp.flat.device
        self.momentum_buffer = torch.zeros_like(self.fp.flat)
        self.sumsq = torch.zeros(1, dtype=torch.float32, device=dev)
        self._steps = 0
        self.hyper = self._hyper_host = None   # device copy of the step's scalars (use_device_hyper: hipGraph mode)
        # data parallel: the all-reduce leaves the SUM over ranks in fp.grad; the mean (DDP semantics) is taken inside
        # the optimizer kernel (g * grad_scale) instead of one more pass over the gradient buffer
        self.grad_scale = 1.0

    def zero_grad(self, set_to_none=True):
        # the reference passes set_to_none=True (nnUNetTrainer.py:901); flat gradient views must persist, so zero
        self.fp.zero_grad()

    def grad_norm(self):
        """Device scalar: the global gradient 2-norm of the last step (before clipping)."""
        return self.sumsq.sqrt() * self.grad_scale

    def _hyper_values(self):
        g = self.param_groups[0]
        return (float(g['lr']), float(g['momentum']), float(g['weight_decay']), float(self.max_grad_norm or 0.0),
                float(self.grad_scale), 1.0 if self._steps == 0 else 0.0)

    def use_device_hyper(self):
        """hipGraph mode (trainer.train_step replayed as one graph launch): the step reads lr / momentum / weight decay /
        clip norm / grad_scale / first-step flag from a 6-float device array (mvd_sgd_nesterov_step_dev), refreshed by
        sync_hyper() between replays, so the captured step follows the PolyLR schedule without re-capture."""
        if self.hyper is None:
            self.hyper = torch.zeros(6, dtype=torch.float32, device=self.fp.flat.device)
            self._hyper_host = None
        self.sync_hyper()

    def sync_hyper(self):
        """Host -> device copy of the step's scalars when one of them changed (outside a capture: once per epoch)."""
        if self.hyper is None:
            return
        v = self._hyper_values()
        if v != self._hyper_host:
            self.hyper.copy_(torch.tensor(v, dtype=torch.float32))
            self._hyper_host = v

    def note_replayed_step(self):
        """A graph replay ran the captured step(): keep the host-side step counter (state_dict, first-step flag) true."""
        self._steps += 1

    def step(self):
        fp, g = self.fp, self.param_groups[0]
        if not g['params'][0].is_cuda:
            raise RuntimeError("FusedSGDNesterov runs on the MI355X only (no CPU path)")
        s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        n = fp.numel
        dev = fp.flat.device
        ws = ops._Workspace.get(query("mvd_sumsq_workspace_bytes", n), dev)
        P = lambda t: ctypes.c_void_p(t.data_ptr())
        if (self.max_grad_norm and self.max_grad_norm > 0) or self.hyper is not None:
            call("mvd_grad_sumsq", P(fp.grad), P(self.sumsq), n, P(ws), ws.numel(), s)
        if self.hyper is not None:
            if not torch.cuda.is_current_stream_capturing():
                self.sync_hyper()
            call("mvd_sgd_nesterov_step_dev", P(fp.flat), P(fp.grad), P(self.momentum_buffer), P(self.sumsq), n,
                 P(self.hyper), s)
        else:
            call("mvd_sgd_nesterov_step", P(fp.flat), P(fp.grad), P(self.momentum_buffer), P(self.sumsq), n,
                 float(g['lr']), float(g['momentum']), float(g['weight_decay']), float(self.max_grad_norm or 0.0),
                 float(self.grad_scale), 1 if self._steps == 0 else 0, s)
        self._steps += 1
        # the update went through a raw pointer: new weight epoch + every cached packed weight rebuilt in one launch
        ops.repack_all(self.fp)

    def state_dict(self):
        return {'momentum_buffer': self.momentum_buffer.clone(), 'steps': self._steps, 'layout': self.fp.layout(),
                'param_groups': [{k: v for k, v in self.param_groups[0].items() if k != 'params'}]}

    def load_state_dict(self, sd):
        """The momentum is ONE flat buffer laid out like FlatParams.flat, so it only means something together with its
        layout.  Same layout: copied.  Another layout with unique names on both sides that cover the same parameters
        (same names and shapes, another order): every parameter's slice is moved to its place here.  Anything else
        raises.  A state without 'layout' (written before the signature existed) is TRUSTED when its size matches."""
        self.momentum_buffer.copy_(_place_flat_state(sd['momentum_buffer'], sd.get('layout'), self.fp, 'momentum'))
        self._steps = sd['steps']
        self.param_groups[0].update(sd['param_groups'][0])


class FusedAdam:
    """torch.nn.utils.clip_grad_norm_(params, max_grad_norm) + torch.optim.Adam / AdamW (amsgrad optional) on the flat
    buffers: mvd_grad_sumsq + mvd_adam_step (variants/optimizer/nnUNetTrainerAdam.py:10-13, :22-24).  Same surface as
    FusedSGDNesterov.  The step's scalars ALWAYS live on the device: `hyper` (8 doubles written here, 16 floats the library
    derives per step) and the int64 counter `step_dev`, which the bias correction reads; `_steps` is its host mirror."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False,
                 decoupled_weight_decay=False, max_grad_norm=12.0):
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"Invalid beta parameters: {betas}")
        self.fp = params if isinstance(params, FlatParams) else FlatParams(list(params))
        self.param_groups = [{'lr': lr, 'betas': tuple(betas), 'eps': eps, 'weight_decay': weight_decay,
                              'amsgrad': bool(amsgrad), 'decoupled_weight_decay': bool(decoupled_weight_decay),
                              'params': self.fp.params}]
        self.max_grad_norm = max_grad_norm
        dev = self.fp.flat.device
        self.exp_avg = torch.zeros_like(self.fp.flat)
        self.exp_avg_sq = torch.zeros_like(self.fp.flat)
        self.max_exp_avg_sq = torch.zeros_like(self.fp.flat) if amsgrad else None
        self.sumsq = torch.zeros(1, dtype=torch.float32, device=dev)
        self.hyper = torch.zeros(16, dtype=torch.float64, device=dev)
        self.step_dev = torch.zeros(1, dtype=torch.int64, device=dev)
        self._hyper_host = None
        self._steps = 0
        self.grad_scale = 1.0   # data parallel: see FusedSGDNesterov

    def zero_grad(self, set_to_none=True):
        self.fp.zero_grad()

    def grad_norm(self):
        """Device scalar: the global gradient 2-norm of the last step (before clipping)."""
        return self.sumsq.sqrt() * self.grad_scale

    def _hyper_values(self):
        g = self.param_groups[0]
        return (float(g['lr']), float(g['betas'][0]), float(g['betas'][1]), float(g['eps']), float(g['weight_decay']),
                float(self.max_grad_norm or 0.0), float(self.grad_scale), 0.0)

    def use_device_hyper(self):
        """hipGraph mode needs nothing more here: the scalars are on the device in eager mode too."""
        self.sync_hyper()

    def sync_hyper(self):
        """Host -> device copy of the scalars when one of them changed (never inside a capture)."""
        v = self._hyper_values()
        if v != self._hyper_host:
            self.hyper[:8].copy_(torch.tensor(v, dtype=torch.float64))
            self._hyper_host = v

    def note_replayed_step(self):
        """A graph replay ran the captured step(): the device counter moved, the host mirror follows."""
        self._steps += 1

    def step(self):
        fp, g = self.fp, self.param_groups[0]
        if not g['params'][0].is_cuda:
            raise RuntimeError("FusedAdam runs on the MI355X only (no CPU path)")
        s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        n = fp.numel
        ws = ops._Workspace.get(query("mvd_sumsq_workspace_bytes", n), fp.flat.device)
        P = lambda t: ctypes.c_void_p(t.data_ptr())
        if not torch.cuda.is_current_stream_capturing():
            self.sync_hyper()
        call("mvd_grad_sumsq", P(fp.grad), P(self.sumsq), n, P(ws), ws.numel(), s)
        call("mvd_adam_step", P(fp.flat), P(fp.grad), P(self.exp_avg), P(self.exp_avg_sq),
             P(self.max_exp_avg_sq) if self.max_exp_avg_sq is not None else None, P(self.sumsq), n, P(self.hyper),
             P(self.step_dev), 1 if g['decoupled_weight_decay'] else 0, s)
        self._steps += 1
        ops.repack_all(self.fp)

    def _buffers(self):
        b = [('exp_avg', self.exp_avg), ('exp_avg_sq', self.exp_avg_sq)]
        if self.max_exp_avg_sq is not None:
            b.append(('max_exp_avg_sq', self.max_exp_avg_sq))
        return b

    def state_dict(self):
        sd = {k: t.clone() for k, t in self._buffers()}
        sd.update(steps=self._steps, layout=self.fp.layout(),
                  param_groups=[{k: v for k, v in self.param_groups[0].items() if k != 'params'}])
        return sd

    def load_state_dict(self, sd):
        """The project's own format: flat buffers with their layout signature, matched like FusedSGDNesterov's momentum
        (same layout copied, a permuted one matched by name, anything else raises before anything is written)."""
        missing = [k for k, _ in self._buffers() if k not in sd]
        if missing:
            raise ValueError(f"optimizer state: no {missing} in the saved state (amsgrad = "
                             f"{self.param_groups[0]['amsgrad']} here)")
        placed = [(t, _place_flat_state(sd[k], sd.get('layout'), self.fp, k)) for k, t in self._buffers()]
        for t, src in placed:
            t.copy_(src)
        self._set_steps(int(sd['steps']))
        self.param_groups[0].update(sd['param_groups'][0])

    def _set_steps(self, steps):
        self._steps = steps
        self.step_dev.fill_(steps)

    # -- torch.optim.Adam(W).state_dict() <-> this optimizer ------------------------------------------------------
    def _index_of(self, named_parameters):
        """For every (name, parameter) in network.parameters() order: its index in the flat layout, by name where the
        layout has names, by identity otherwise."""
        named = [(n, p) for n, p in named_parameters if p.requires_grad]
        by_name = {n: j for j, n in enumerate(self.fp.names) if n is not None}
        by_id = {id(p): j for j, p in enumerate(self.fp.params)}
        idx = [by_name[n] if n in by_name else by_id.get(id(p)) for n, p in named]
        if None in idx or sorted(idx) != list(range(len(self.fp.params))):
            raise ValueError("optimizer state: the named parameters do not cover the parameters of this optimizer "
                             f"one to one ({len(named)} given, {len(self.fp.params)} here)")
        return idx

    def to_torch_state_dict(self, named_parameters):
        """torch.optim.Adam(W)(network.parameters()).state_dict(): state[i] in network.parameters() order."""
        g = self.param_groups[0]
        idx = self._index_of(named_parameters)
        state = {}
        if self._steps > 0:
            for i, j in enumerate(idx):
                p, o = self.fp.params[j], self.fp.offsets[j]
                state[i] = {'step': torch.tensor(float(self._steps), dtype=torch.float32)}
                for k, t in self._buffers():
                    state[i][k] = t[o:o + p.numel()].view(p.shape).clone()
        group = {'lr': g['lr'], 'betas': tuple(g['betas']), 'eps': g['eps'], 'weight_decay': g['weight_decay'],
                 'amsgrad': g['amsgrad'], 'maximize': False, 'foreach': None, 'capturable': False,
                 'differentiable': False, 'fused': None, 'decoupled_weight_decay': g['decoupled_weight_decay'],
                 'params': list(range(len(idx)))}
        return {'state': state, 'param_groups': [group]}

    def load_torch_state_dict(self, sd, named_parameters):
        """The reverse: a reference checkpoint's `optimizer_state`.  Per-parameter `step` values that differ from each
        other cannot be one device counter and raise."""
        idx = self._index_of(named_parameters)
        state = sd['state']
        if len(sd['param_groups']) != 1:
            raise ValueError(f"optimizer state: {len(sd['param_groups'])} param_groups, this optimizer holds one")
        if state and set(state) != set(range(len(idx))):
            raise ValueError(f"optimizer state: state of {len(state)} parameters, this optimizer holds {len(idx)}")
        steps = {float(st['step']) for st in state.values()}
        if len(steps) > 1:
            raise ValueError(f"optimizer state: per-parameter step counts differ ({sorted(steps)[:4]}...); one fused "
                             "update has one step count")
        new = [(t, torch.zeros_like(t)) for _k, t in self._buffers()]
        for i, j in enumerate(idx if state else []):
            p, o = self.fp.params[j], self.fp.offsets[j]
            for (k, _t), (_, dst) in zip(self._buffers(), new):
                if k not in state[i]:
                    raise ValueError(f"optimizer state: no '{k}' for parameter {i} (amsgrad = "
                                     f"{self.param_groups[0]['amsgrad']} here)")
                if tuple(state[i][k].shape) != tuple(p.shape):
                    raise ValueError(f"optimizer state: '{k}' of parameter {i} has shape {tuple(state[i][k].shape)}, "
                                     f"the parameter {tuple(p.shape)}")
                dst[o:o + p.numel()] = state[i][k].reshape(-1).to(dst)
        for t, src in new:
            t.copy_(src)
        self._set_steps(int(steps.pop()) if steps else 0)
        tg = sd['param_groups'][0]
        self.param_groups[0].update({k: tg[k] for k in ('lr', 'betas', 'eps', 'weight_decay') if k in tg})


class CosineAnnealingLR:
    """torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, T_max) stepped with the epoch, as the reference's
    nnUNetTrainerCosAnneal does (variants/lr_schedule/nnUNetTrainerCosAnneal.py:11; nnUNetTrainer.py:880): the closed form
    eta_min + (base_lr - eta_min) * (1 + cos(pi * epoch / T_max)) / 2."""

    def __init__(self, optimizer, T_max: int, eta_min: float = 0.0):
        self.optimizer, self.T_max, self.eta_min = optimizer, T_max, eta_min
        self.base_lrs = [g['lr'] for g in optimizer.param_groups]
        self.ctr = 0
        self.step()

    def step(self, current_step=None):
        if current_step is None or current_step == -1:
            current_step = self.ctr
            self.ctr += 1
        for param_group, base_lr in zip(self.optimizer.param_groups, self.base_lrs):
            param_group['lr'] = self.eta_min + (base_lr - self.eta_min) * (1 + math.cos(math.pi * current_step / self.T_max)) / 2


class PolyLRScheduler:
    """polylr.py:4-20: lr = initial_lr * (1 - step/max_steps) ** exponent, stepped once per epoch
    (nnUNetTrainer.py:880)."""

    def __init__(self, optimizer, initial_lr: float, max_steps: int, exponent: float = 0.9, current_step: int = None):
        self.optimizer, self.initial_lr, self.max_steps, self.exponent = optimizer, initial_lr, max_steps, exponent
        self.ctr = 0
        self.step(current_step if current_step is not None else -1)

    def step(self, current_step=None):
        if current_step is None or current_step == -1:
            current_step = self.ctr
            self.ctr += 1
        new_lr = self.initial_lr * (1 - current_step / self.max_steps) ** self.exponent
        for param_group in self.optimizer.param_groups:
            param_group['lr'] = new_lr
