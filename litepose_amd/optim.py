"""``torch.optim.Adam`` / ``torch.optim.SGD`` on the library's update kernels (include/litepose_amd.h, "optimizers").

One ``lp_optim_adam`` / ``lp_optim_sgd`` call per parameter group and ``step()``: every tensor of the group in a handful
of launches whose arguments carry the pointers.  ``lr`` is read from a device fp64 scalar when the launches run and the step
counts live in one device array per group, so a ``step()`` can sit inside a captured graph and a scheduler
(``MultiStepLR`` writes ``param_groups[i]['lr']``) still takes effect: ``sync_hyperparameters()`` uploads the value when it
has changed.  The other hyperparameters travel by value in the launch; changing one after a capture is refused at the next
``sync_hyperparameters()`` -- before anything is written -- until ``forget_captures()`` (``CapturedStep.invalidate()``
calls it) has cleared the marks.

A captured graph holds the addresses of the state tensors, of the ``lr`` scalars and of the step arrays.  ``generation``
counts the events after which a graph captured earlier no longer describes the optimizer: ``load_state_dict()`` (every state
tensor and device scalar is a new one), ``add_param_group()`` after construction (a group the graph does not update, without
state yet) and ``forget_captures()``.  ``core.trainer.CapturedStep`` compares it before every step and captures again when it
has moved.  Nothing else moves it: ``state_dict()``, ``zero_grad()``, a changed ``lr`` and ``sync_hyperparameters()`` leave
every address where it was.

``state_dict()`` / ``load_state_dict()`` speak torch's format (per parameter ``step``, ``exp_avg``, ``exp_avg_sq`` or
``momentum_buffer``, plus ``param_groups``), in both directions with the torch optimizer of the same name on the same
parameters; both work on CPU parameters, ``step()`` needs the GPU."""
import ctypes as C

import torch

from . import _native as nv


def _ptr_array(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


class _NativeOptimizer(torch.optim.Optimizer):
    _BY_VALUE = ()               # keys of a param group that travel by value in the launch
    _SLOTS = ()                  # per-parameter state tensors shaped like the parameter

    def __init__(self, params, defaults):
        self._constructed = False
        super().__init__(params, defaults)
        self._native = {}        # id(group) -> dict(steps=[n] fp32 | None, lr=0-dim fp64, lr_host, captured=by-value key | None)
        self.generation = 0      # moves when a graph captured earlier no longer describes this optimizer (module docstring)
        self._constructed = True

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        for p in self.param_groups[-1]['params']:
            what = ('float32 parameters only, got %s' % p.dtype if p.dtype != torch.float32 else
                    'dense parameters only, got %s' % p.layout if p.layout != torch.strided else None)
            if what:
                self.param_groups.pop()                  # a refused group is no group, and no event
                raise TypeError('%s: %s' % (type(self).__name__, what))
        if self._constructed:
            self.generation += 1

    # ---- per-group device state ----
    def _group_native(self, group):
        ns = self._native.get(id(group))
        if ns is None:
            dev = group['params'][0].device
            ns = dict(lr=torch.tensor(float(group['lr']), dtype=torch.float64, device=dev), lr_host=float(group['lr']),
                      steps=None, captured=None, cache=None)
            self._native[id(group)] = ns
        return ns

    def _steps(self, group):
        """The group's step array ([len(params)] fp32 on the parameters' device); a parameter's state['step'] is a view."""
        ns = self._group_native(group)
        if ns['steps'] is None:
            ns['steps'] = torch.zeros(len(group['params']), dtype=torch.float32, device=group['params'][0].device)
        return ns['steps']

    def _init_state(self, group, i, p):
        st = self.state[p]
        if not st:
            if p.is_cuda and torch.cuda.is_current_stream_capturing():
                raise RuntimeError('optimizer state cannot be created inside a capture: run one eager step() first')
            st['step'] = self._steps(group)[i]
            for key in self._slots(group):
                st[key] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        return st

    def _slots(self, group):
        return self._SLOTS

    def _by_value(self, group):
        return tuple(group[k] for k in self._BY_VALUE)

    def forget_captures(self):
        """Clear every group's mark of a captured ``step()`` and move ``generation``: the graphs that held the by-value
        hyperparameters are the caller's to drop (``CapturedStep.invalidate()`` does both)."""
        for ns in self._native.values():
            ns['captured'] = None
        self.generation += 1

    def sync_hyperparameters(self):
        """Refuse a by-value hyperparameter that differs from what a captured ``step()`` holds -- for every group, before
        anything is written -- then write every group's ``lr`` into its device scalar where the value has changed."""
        for group in self.param_groups:
            ns = self._group_native(group)
            if ns['captured'] is not None and ns['captured'] != self._by_value(group):
                raise RuntimeError('%s: %s changed after step() was captured (%r -> %r): these travel by value in the '
                                   'captured launches; call CapturedStep.invalidate() (or forget_captures() on an optimizer '
                                   'captured by hand) to capture again'
                                   % (type(self).__name__, '/'.join(self._BY_VALUE), ns['captured'], self._by_value(group)))
        for group in self.param_groups:
            ns = self._group_native(group)
            lr = float(group['lr'])
            if lr != ns['lr_host']:
                ns['lr'].fill_(lr)
                ns['lr_host'] = lr

    # ---- the step ----
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        capturing = torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()
        if not capturing:
            self.sync_hyperparameters()
        for group in self.param_groups:
            active = [(i, p) for i, p in enumerate(group['params']) if p.grad is not None]
            if not active:
                continue
            for _, p in active:
                if not p.is_cuda:
                    raise RuntimeError('%s.step(): parameters must live on the GPU' % type(self).__name__)
                if p.grad.is_sparse or p.grad.dtype != torch.float32:
                    raise RuntimeError('%s.step(): dense float32 gradients only' % type(self).__name__)
                if not p.is_contiguous():
                    raise RuntimeError('%s.step(): contiguous parameters only' % type(self).__name__)
            ns = self._group_native(group)
            if capturing:
                ns['captured'] = self._by_value(group)
            states = [self._init_state(group, i, p) for i, p in active]
            self._launch(group, ns, active, states)
        return loss

    def _static_arrays(self, group, ns, active, states):
        """Host arrays that do not change from step to step (parameters, state tensors, lengths), kept per active set."""
        key = tuple(i for i, _ in active)
        c = ns['cache']
        if c is None or c['key'] != key or c['ptrs'] != [p.data_ptr() for _, p in active]:
            c = dict(key=key, ptrs=[p.data_ptr() for _, p in active], params=_ptr_array([p for _, p in active]),
                     numel=(C.c_int64 * len(active))(*[p.numel() for _, p in active]),
                     slots=[_ptr_array([st[k] for st in states]) for k in self._slots(group)],
                     index=None if len(active) == len(group['params'])
                     else torch.tensor(key, dtype=torch.int64, device=active[0][1].device))
            ns['cache'] = c
        return c

    @staticmethod
    def _grads(active):
        grads = [p.grad if p.grad.is_contiguous() else p.grad.contiguous() for _, p in active]
        return grads, _ptr_array(grads)

    # ---- torch's format ----
    def state_dict(self):
        """torch's layout; ``step`` as torch's own default keeps it: a 0-dim float32 CPU tensor per parameter."""
        def own(k, v):
            if not torch.is_tensor(v):
                return v
            return v.detach().cpu().clone() if k == 'step' else v.detach().clone()

        sd = super().state_dict()                # its per-parameter dicts are the live ones: copy, never edit
        sd['state'] = {i: {k: own(k, v) for k, v in st.items()} for i, st in sd['state'].items()}
        return sd

    def load_state_dict(self, state_dict):
        """torch's loader, then the library's layout again.  Every state tensor, ``lr`` scalar and step array is a NEW
        tensor afterwards and the marks of a captured ``step()`` are gone: ``generation`` moves."""
        super().load_state_dict(state_dict)
        self._native = {}
        self.generation += 1
        for group in self.param_groups:
            steps = None
            for i, p in enumerate(group['params']):
                st = self.state.get(p)
                if not st:
                    continue
                if steps is None:
                    steps = self._steps(group)
                steps[i] = float(st.get('step', 0.0))
                st['step'] = steps[i]
                for k in self._slots(group):
                    v = st.get(k)
                    if v is None:                               # torch's SGD keeps None until the first step
                        v = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st[k] = v.detach().to(device=p.device, dtype=torch.float32, copy=True).contiguous()   # torch's loader aliases
                for k in [k for k in st if k != 'step' and k not in self._slots(group)]:
                    del st[k]


class Adam(_NativeOptimizer):
    """``torch.optim.Adam(params, lr, betas, eps, weight_decay)`` (no amsgrad, no maximize, L2 weight decay) as one
    ``lp_optim_adam`` call per parameter group."""
    _BY_VALUE = ('betas', 'eps', 'weight_decay')
    _SLOTS = ('exp_avg', 'exp_avg_sq')

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0):
        if not 0.0 <= lr:
            raise ValueError('Invalid learning rate: %r' % (lr,))
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError('Invalid betas: %r' % (betas,))
        if not 0.0 <= eps:
            raise ValueError('Invalid epsilon value: %r' % (eps,))
        if not 0.0 <= weight_decay:
            raise ValueError('Invalid weight_decay value: %r' % (weight_decay,))
        # the keys of torch.optim.Adam's param_groups, so that either optimizer loads the other's state_dict unchanged
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False,
                                      maximize=False, foreach=None, capturable=False, differentiable=False, fused=None,
                                      decoupled_weight_decay=False))

    def _by_value(self, group):
        return (tuple(float(b) for b in group['betas']), float(group['eps']), float(group['weight_decay']))

    def _launch(self, group, ns, active, states):
        if group.get('amsgrad') or group.get('maximize') or group.get('decoupled_weight_decay'):
            raise RuntimeError('litepose_amd.optim.Adam: amsgrad, maximize and decoupled weight decay are not supported')
        c = self._static_arrays(group, ns, active, states)
        grads, gptr = self._grads(active)
        steps = self._steps(group)
        sub = steps if c['index'] is None else steps[c['index']]          # skipped parameters: their step does not advance
        (b1, b2), eps, wd = self._by_value(group)
        nv.check(nv.lib().lp_optim_adam(len(active), c['params'], gptr, c['slots'][0], c['slots'][1], c['numel'],
                                        nv.dptr(sub), nv.dptr(ns['lr']), b1, b2, eps, wd, nv.stream_ptr()), 'lp_optim_adam')
        if c['index'] is not None:
            steps[c['index']] = sub


class SGD(_NativeOptimizer):
    """``torch.optim.SGD(params, lr, momentum, weight_decay, nesterov)`` with dampening 0 as one ``lp_optim_sgd`` call per
    parameter group."""
    _BY_VALUE = ('momentum', 'weight_decay', 'nesterov')

    def __init__(self, params, lr=1e-3, momentum=0, weight_decay=0, nesterov=False):
        if not 0.0 <= lr:
            raise ValueError('Invalid learning rate: %r' % (lr,))
        if momentum < 0.0:
            raise ValueError('Invalid momentum value: %r' % (momentum,))
        if weight_decay < 0.0:
            raise ValueError('Invalid weight_decay value: %r' % (weight_decay,))
        if nesterov and momentum <= 0:
            raise ValueError('Nesterov momentum requires a momentum')
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=0, weight_decay=weight_decay, nesterov=nesterov,
                                      maximize=False, foreach=None, differentiable=False, fused=None))

    def _slots(self, group):
        return ('momentum_buffer',) if group['momentum'] != 0 else ()

    def _by_value(self, group):
        return (float(group['momentum']), float(group['weight_decay']), bool(group['nesterov']))

    def _init_state(self, group, i, p):
        st = self.state[p]
        if self._slots(group) and st.get('momentum_buffer') is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError('optimizer state cannot be created inside a capture: run one eager step() first')
            st['momentum_buffer'] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        return st

    def _launch(self, group, ns, active, states):
        if group.get('dampening') or group.get('maximize'):
            raise RuntimeError('litepose_amd.optim.SGD: dampening and maximize are not supported')
        c = self._static_arrays(group, ns, active, states)
        grads, gptr = self._grads(active)
        mu, wd, nesterov = self._by_value(group)
        nv.check(nv.lib().lp_optim_sgd(len(active), c['params'], gptr, c['slots'][0] if c['slots'] else None, c['numel'],
                                       nv.dptr(ns['lr']), mu, wd, int(nesterov), nv.stream_ptr()), 'lp_optim_sgd')

    def load_state_dict(self, state_dict):                      # no step counts here
        torch.optim.Optimizer.load_state_dict(self, state_dict)
        self._native = {}
        self.generation += 1
        for group in self.param_groups:
            for p in group['params']:
                st = self.state.get(p)
                if st and st.get('momentum_buffer') is not None:
                    st['momentum_buffer'] = st['momentum_buffer'].detach().to(device=p.device, dtype=torch.float32,
                                                                              copy=True).contiguous()


def get_optimizer(cfg, model):
    """lib/utils/utils.py:77-93 over this module's classes: ``cfg.TRAIN.OPTIMIZER`` 'sgd' (LR, MOMENTUM, WD, NESTEROV) or
    'adam' (LR); None for any other name, as there."""
    optimizer = None
    if cfg.TRAIN.OPTIMIZER == 'sgd':
        optimizer = SGD(model.parameters(), lr=cfg.TRAIN.LR, momentum=cfg.TRAIN.MOMENTUM, weight_decay=cfg.TRAIN.WD,
                        nesterov=cfg.TRAIN.NESTEROV)
    elif cfg.TRAIN.OPTIMIZER == 'adam':
        optimizer = Adam(model.parameters(), lr=cfg.TRAIN.LR)
    return optimizer
