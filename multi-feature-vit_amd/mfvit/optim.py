"""Multi-tensor optimizers on the HIP path: torch.optim.Optimizer subclasses with the reference's
constructor signatures whose ``step()`` is one or two kernel launches over a device-resident chunk table.

State layout = the reference's / torch's, so optimizer state dicts move both ways between this package and the reference drivers
(MAIN_MOCO:461-467 saves ``optimizer.state_dict()``, its resume path loads it):
  LARS (OPT:10-43)            state[p] = {'mu'}
  Adam / AdamW (torch.optim)  state[p] = {'step' (f32 scalar tensor), 'exp_avg', 'exp_avg_sq'}
  SGD (torch.optim)           state[p] = {'momentum_buffer'}
The device chunk tables are runtime caches of raw addresses: they live on the optimizer object (never inside ``param_groups``,
which ``state_dict()`` pickles), are keyed by every address a row holds (parameter, gradient, both state tensors), and are dropped by
``load_state_dict``.

``clip_grad_norm_`` / ``grad_norm`` (torch.nn.utils.clip_grad_norm_) run over the same tables: they take the optimizer, not the parameters.  ``SAM`` (davda54/sam's wrapper: sharpness-aware minimisation, adaptive or not) perturbs and restores the
parameters over tables of its own, whose one state column is the scratch copy ``old_p``; what it saves and loads is the base optimizer's state.
"""
import torch

from . import _lib
from ._lib import check, lib, ptr, stream

CHUNK = 1 << 14          # elements per table row = per workgroup (45 M parameters: ~2,800 workgroups of 256 threads)


def _bump_versions(params):
    """The kernels write parameters through raw pointers: tell autograd (saved-tensor checks) and the encoders' weight-shadow
    caches (keyed on the parameter versions) that the data changed."""
    torch._C._increment_version(list(params))


class _TableOptimizer(torch.optim.Optimizer):
    state_names = ("s0",)          # names of the per-parameter state tensors, in table-column order

    # ---- runtime caches (never pickled: Optimizer.__getstate__ keeps defaults / state / param_groups only)
    def _cache(self):
        c = self.__dict__.get("_mfvit_cache")
        if c is None:
            c = self.__dict__["_mfvit_cache"] = {}
        return c

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._cache().clear()      # the loaded state tensors live at new addresses
        for g in self.param_groups:     # checkpoints written by round-1 builds carried these runtime keys
            g.pop("_mfvit_live", None)
            g.pop("_mfvit_tables", None)

    def _ensure_state(self, p):
        st = self.state[p]
        for name in self.state_names:
            t = st.get(name)
            if t is None:
                st[name] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            elif (not t.is_cuda or t.device != p.device or t.dtype != torch.float32 or not t.is_contiguous()
                  or t.shape != p.shape):
                st[name] = t.to(device=p.device, dtype=torch.float32).reshape(p.shape).contiguous()
        return st

    def _table(self, gi, group):
        """(table tensor, ntensors, live params) for the params of `group` that have gradients; rebuilt when any address changes."""
        cache = self._cache().setdefault(gi, {})
        # Fast path (the host sets the pace of a small-batch step: tools/host_profile.py measured 1.8 ms of Python per optimizer step here,
        # of a 6.8 ms step at 16 pairs): the same parameter objects with the same addresses as the last call - parameter, gradient, every state
        # tensor - mean the same table.  One flat list of integers is compared; nothing else is touched.
        params = group["params"]
        last = cache.get("last")
        if last is not None and len(last[0]) == len(params) and last[4] == len(self.state):     # (state.clear() / a new parameter: the slow path)
            names = self.state_names
            sig = []
            try:
                for p, st in zip(params, last[1]):
                    g = p.grad
                    sig.append(p.data_ptr())
                    sig.append(0 if g is None else g.data_ptr())
                    if st is not None:
                        for n in names:
                            sig.append(st[n].data_ptr())
            except (KeyError, AttributeError):
                sig = None
            if sig is not None and sig == last[2] and all(a is b for a, b in zip(params, last[0])):
                return last[3]
        ps = [p for p in params if p.grad is not None]
        if not ps:
            return None, 0, ps
        keys = []
        for p in ps:
            if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous() or p.grad.dtype != torch.float32:
                raise _lib.MfvitError("the HIP optimizers need contiguous f32 parameters and gradients on the GPU")
            if not p.grad.is_contiguous():
                p.grad = p.grad.contiguous()
            st = self._ensure_state(p)
            keys.append((p.data_ptr(), p.grad.data_ptr(), p.numel()) + tuple(st[n].data_ptr() for n in self.state_names))
        key = tuple(keys)
        # Gradients are re-created every step (zero_grad(set_to_none=True)); the caching allocator hands the same few addresses out
        # in a cycle, so keep a table per address pattern instead of rebuilding (a ~700-row Python loop + an upload) whenever it
        # changes.  The upload goes through pinned memory and does not block the host: a pageable cudaMemcpy here would wait for the
        # whole backward still queued on the stream and leave the GPU idle until the host has caught up again (measured: 1.9 ms of
        # idle GPU per step).
        tables = cache.setdefault("tables", {})
        hit = tables.get(key)
        if hit is None:
            rows = []
            for tid, p in enumerate(ps):
                st = self.state[p]
                n = p.numel()
                s0 = st[self.state_names[0]].data_ptr()
                s1 = st[self.state_names[1]].data_ptr() if len(self.state_names) > 1 else 0
                for a in range(0, n, CHUNK):
                    c = min(CHUNK, n - a)
                    rows.append([tid, p.data_ptr() + 4 * a, p.grad.data_ptr() + 4 * a, s0 + 4 * a, s1 + 4 * a if s1 else 0, c,
                                 self._flag(p, group)])
            host = torch.tensor(rows, dtype=torch.int64).pin_memory()
            if len(tables) >= 8:
                tables.clear()
            dev = host.to(ps[0].device, non_blocking=True)
            # (column 0 as int32: the per-row tensor index of mfvit_grad_clip_coef, made on the device from the table just uploaded)
            hit = tables[key] = (dev, len(ps), host, dev[:, 0].to(torch.int32))   # keep the pinned source alive
        out = (hit[0], hit[1], ps)
        cache["row_tensor"] = hit[3]     # belongs to `out`: the fast path above hands `out` back only while nothing has changed
        # signature of this call for the fast path: the state dicts of the live parameters (None for a parameter without a gradient)
        sts = [self.state[p] if p.grad is not None else None for p in params]
        sig = []
        for p, st in zip(params, sts):
            sig.append(p.data_ptr())
            sig.append(0 if p.grad is None else p.grad.data_ptr())
            if st is not None:
                for n in self.state_names:
                    sig.append(st[n].data_ptr())
        cache["last"] = (list(params), sts, sig, out, len(self.state))
        return out

    def _flag(self, p, group):
        return 0

    # ``optimizer.before_group = fn(group_index)`` runs before the kernels of each param group are queued: the data-parallel driver
    # joins only that group's gradient exchange there (GradSync.finish(owner)), so the update of the arenas whose all-reduce is
    # complete overlaps the exchanges still on the links.
    before_group = None

    def _pre(self, gi):
        cb = self.__dict__.get("before_group")
        if cb is not None:
            cb(gi)

    @torch.no_grad()
    def unscale_(self, inv_scale, found_inf):
        """GradScaler.unscale_: g *= inv_scale for every gradient of this optimizer; found_inf (device f32[1]) is set to 1 when a
        gradient held an inf / nan (mfvit_amp_unscale)."""
        for gi, g in enumerate(self.param_groups):
            self._pre(gi)
            table, nt, _ = self._table(gi, g)
            if table is None:
                continue
            check(lib().mfvit_amp_unscale(ptr(table), table.shape[0], float(inv_scale), ptr(found_inf), stream()), "mfvit_amp_unscale")

    def clip_grad_norm_(self, max_norm, norm_type=2.0, error_if_nonfinite=False, per_tensor=False):
        """``clip_grad_norm_(self, ...)``: one total over every param group of this optimizer."""
        return clip_grad_norm_(self, max_norm, norm_type, error_if_nonfinite, per_tensor)


class LARS(_TableOptimizer):
    """LARS optimizer, no rate scaling or weight decay for parameters <= 1D (OPT:10-43)."""
    state_names = ("mu",)

    def __init__(self, params, lr=0, weight_decay=0, momentum=0.9, trust_coefficient=0.001):
        defaults = dict(lr=lr, weight_decay=weight_decay, momentum=momentum, trust_coefficient=trust_coefficient)
        super().__init__(params, defaults)

    def _flag(self, p, group):
        return 1 if p.ndim > 1 else 0

    @torch.no_grad()
    def step(self):
        for gi, g in enumerate(self.param_groups):
            self._pre(gi)
            table, nt, live = self._table(gi, g)
            if table is None:
                continue
            norms = torch.empty(2 * nt, device=table.device, dtype=torch.float32)
            check(lib().mfvit_lars_step(ptr(table), table.shape[0], nt, ptr(norms), float(g["lr"]), float(g["weight_decay"]),
                                        float(g["momentum"]), float(g["trust_coefficient"]), stream()), "mfvit_lars_step")
            _bump_versions(live)


class Adam(_TableOptimizer):
    """torch.optim.Adam semantics (L2 weight decay folded into the gradient)."""
    state_names = ("exp_avg", "exp_avg_sq")
    decoupled = False

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    def _flag(self, p, group):
        return 1 if self.decoupled else 0

    def _bump_steps(self, gi, live):
        """state[p]['step'] += 1 for the live parameters; returns the values BEFORE the increment.  The per-parameter f32 scalars of torch.optim
        (host tensors) are 0-dim views of ONE host vector per param group, so the increment is one add on that vector and the values one
        tolist() - 324 scalar tensors bumped one by one (`_foreach_add_` has no fast path on the CPU) were 0.5 ms of host time per step.  A 'step'
        somebody replaced (a loaded state dict, a torch optimizer's state) is taken at its value and moved into the shared vector."""
        cache = self._cache().setdefault(("steps", gi), {})
        views = cache.get("views")
        if cache.get("live") is live:          # (the table's fast path hands the same list object out while nothing has changed)
            sts = cache["sts"]
        else:
            sts = [self.state[p] for p in live]
            cache["live"], cache["sts"] = live, sts
        if views is None or len(views) != len(sts) or any(st.get("step") is not v for st, v in zip(sts, views)):
            vals = []
            for st in sts:
                t = st.get("step")
                vals.append(float(t) if t is not None else 0.0)
            buf = torch.tensor(vals, dtype=torch.float32)
            views = [buf[i] for i in range(len(vals))]
            for st, v in zip(sts, views):
                st["step"] = v
            cache["buf"], cache["views"] = buf, views
        buf = cache["buf"]
        vals = [int(v) for v in buf.tolist()]
        buf += 1.0
        return vals

    @torch.no_grad()
    def step(self):
        for gi, g in enumerate(self.param_groups):
            self._pre(gi)
            table, nt, live = self._table(gi, g)
            if table is None:
                continue
            # per-parameter 'step' like torch.optim (f32 scalar tensors on the host).  One kernel launch serves one step number (bias
            # correction): normally every parameter of the group agrees and the whole table goes out in one launch; otherwise (a parameter
            # whose first gradient arrived later, an unfrozen layer, a loaded torch state dict with mixed steps) the table rows - laid out
            # parameter by parameter - are launched in runs of equal step.
            vals = self._bump_steps(gi, live)
            if vals and vals.count(vals[0]) == len(vals):          # the normal case: one step number, the whole table in one launch
                runs = [[0, table.shape[0], vals[0] + 1]]
            else:
                runs = []                                      # (first table row, rows, step after the increment)
                row = 0
                for p, v in zip(live, vals):
                    nrows = (p.numel() + CHUNK - 1) // CHUNK
                    if runs and runs[-1][2] == v + 1:
                        runs[-1][1] += nrows
                    else:
                        runs.append([row, nrows, v + 1])
                    row += nrows
                assert row == table.shape[0]
            for first, nrows, step in runs:
                check(lib().mfvit_adam_step(ptr(table) + first * table.shape[1] * 8, nrows, float(g["lr"]), float(g["betas"][0]),
                                            float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]), step, stream()), "mfvit_adam_step")
            _bump_versions(live)


class AdamW(Adam):
    """torch.optim.AdamW semantics (decoupled weight decay; default 1e-2 like torch)."""
    decoupled = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)


class SGD(_TableOptimizer):
    """torch.optim.SGD semantics (momentum, L2 weight decay; no dampening / nesterov).  torch initialises 'momentum_buffer' with the
    first update d; a zero buffer gives the same first step (momentum * 0 + d), so the kernel never needs the first-step case."""
    state_names = ("momentum_buffer",)

    def __init__(self, params, lr=1e-3, momentum=0, weight_decay=0, dampening=0, nesterov=False):
        if dampening != 0 or nesterov:
            raise NotImplementedError("the HIP SGD kernel implements the reference's configuration (MAIN_CA:445-448): no dampening, no nesterov")
        # dampening / nesterov are kept in the group so that torch.optim.SGD can load this optimizer's state dict (and vice versa)
        super().__init__(params, dict(lr=lr, momentum=momentum, weight_decay=weight_decay, dampening=0, nesterov=False))

    @torch.no_grad()
    def step(self):
        for gi, g in enumerate(self.param_groups):
            self._pre(gi)
            table, nt, live = self._table(gi, g)
            if table is None:
                continue
            check(lib().mfvit_sgd_step(ptr(table), table.shape[0], float(g["lr"]), float(g["momentum"]), float(g["weight_decay"]), 0,
                                       stream()), "mfvit_sgd_step")
            _bump_versions(live)


# ------------------------------------------------------------------------------------------------ sharpness-aware minimisation
class SAM(_TableOptimizer):
    """davda54/sam's ``SAM(params, base_optimizer, rho=0.05, adaptive=False, **kwargs)`` (Foret et al. 2021; adaptive=True: ASAM, Kwon et al. 2021)
    on the chunk tables.  ``base_optimizer`` is one of this module's CLASSES; ``kwargs`` are its hyperparameters.  ``param_groups`` are the base
    optimizer's own list, with ``rho`` / ``adaptive`` as group keys; ONE norm is taken over all groups.

        loss_fn(model(x), y).backward();  opt.first_step(zero_grad=True)      # w += rho g / |g|   (ASAM: rho w^2 g / | |w| g |)
        loss_fn(model(x), y).backward();  opt.second_step(zero_grad=True)     # w = old_p, then the base optimizer's step on the new gradients

    or ``opt.step(closure)``.  first_step: a norm pass per table (mfvit_sam_norm_partials), one finalize (mfvit_sam_scale), a perturb pass per table
    (mfvit_sam_perturb); second_step: a restore pass per table (mfvit_sam_restore) and the base step.  Both tell the weight-shadow caches that the
    parameters moved.  Nothing waits for the GPU.  With a GradScaler pass ``scaler=`` to both steps and call ``scaler.update()`` afterwards: an
    overflow in either backward moves nothing (decided on the device) and skips the base step.  ``old_p`` is scratch of this object:
    ``state_dict()`` / ``load_state_dict()`` are the base optimizer's, so checkpoints move between SAM and plain runs."""
    state_names = ("old_p",)

    def __init__(self, params, base_optimizer, rho=0.05, adaptive=False, **kwargs):
        if not (isinstance(base_optimizer, type) and issubclass(base_optimizer, _TableOptimizer)) or issubclass(base_optimizer, SAM):
            raise TypeError("mfvit.optim.SAM takes one of the optimizer classes of mfvit.optim (Adam, AdamW, SGD, LARS) as base_optimizer, not "
                            f"{base_optimizer!r}: the device chunk tables the kernels stream over live on the optimizer")
        if not rho >= 0.0:
            raise ValueError(f"Invalid rho, should be non-negative: {rho}")
        super().__init__(params, dict(rho=rho, adaptive=adaptive, **kwargs))
        self.base_optimizer = base_optimizer(self.param_groups, **kwargs)
        self.param_groups = self.base_optimizer.param_groups
        self.defaults.update(self.base_optimizer.defaults)
        self._pending = None       # (tables of the perturbed rows with their live parameters, out2) between first_step and second_step

    def _flag(self, p, group):
        return 1 if group["adaptive"] else 0

    def _table(self, gi, group):
        cache = self._cache().setdefault(gi, {})
        if cache.get("adaptive") != bool(group["adaptive"]):     # the flag column is part of a table
            cache.clear()
            cache["adaptive"] = bool(group["adaptive"])
        return super()._table(gi, group)

    def state_dict(self):
        return self.base_optimizer.state_dict()

    def load_state_dict(self, state_dict):
        mine = [(g["rho"], g["adaptive"]) for g in self.param_groups]
        self.base_optimizer.load_state_dict(state_dict)
        self.param_groups = self.base_optimizer.param_groups
        for g, (rho, adaptive) in zip(self.param_groups, mine):       # a checkpoint of a plain run has no SAM keys: the groups keep theirs
            g.setdefault("rho", rho)
            g.setdefault("adaptive", adaptive)
        self._cache().clear()

    def clip_grad_norm_(self, max_norm, norm_type=2.0, error_if_nonfinite=False, per_tensor=False):
        return self.base_optimizer.clip_grad_norm_(max_norm, norm_type, error_if_nonfinite, per_tensor)

    @torch.no_grad()
    def first_step(self, zero_grad=False, scaler=None):
        if self._pending is not None:
            raise RuntimeError("SAM.first_step() was called twice in a row: the parameters are perturbed, call second_step() first")
        flag = None
        if scaler is not None and scaler.is_enabled():
            dev = next(p for g in self.param_groups for p in g["params"]).device
            flag = scaler._flag(dev)
            self.unscale_(1.0 / scaler.get_scale(), flag)       # not registered with the scaler: these gradients never reach a step
        scratch = self._cache().setdefault("sam", {})
        part = scratch.get("partials")
        tabs, rows = [], 0
        for gi, g in enumerate(self.param_groups):
            self._pre(gi)
            table, _, live = self._table(gi, g)
            if table is None:
                continue
            nrows = table.shape[0]
            if part is None or rows + nrows > part.numel():
                grown = torch.empty(max(1024, rows + nrows, 2 * (0 if part is None else part.numel())), device=table.device, dtype=torch.float32)
                if rows:
                    grown[:rows].copy_(part[:rows])
                part = scratch["partials"] = grown
            check(lib().mfvit_sam_norm_partials(ptr(table), nrows, 1 if g["adaptive"] else 0, part.data_ptr() + 4 * rows, stream()),
                  "mfvit_sam_norm_partials")
            tabs.append((table, live, float(g["rho"])))
            rows += nrows
        out = None
        if tabs:
            out = torch.empty(2, device=part.device, dtype=torch.float32)      # a fresh pair per step: second_step reads out[1]
            check(lib().mfvit_sam_scale(ptr(part), rows, ptr(flag), ptr(out), stream()), "mfvit_sam_scale")
            for table, live, rho in tabs:
                check(lib().mfvit_sam_perturb(ptr(table), table.shape[0], out.data_ptr() + 4, rho, stream()), "mfvit_sam_perturb")
                _bump_versions(live)
        self._pending = (tabs, out)
        if zero_grad:
            self.zero_grad()

    @torch.no_grad()
    def second_step(self, zero_grad=False, scaler=None):
        if self._pending is None:
            raise RuntimeError("SAM.second_step() needs a first_step() before it")
        cb = self.__dict__.get("before_group")
        if cb is not None:
            self.base_optimizer.before_group = cb
        for gi in range(len(self.param_groups)):
            self._pre(gi)
        if scaler is not None and scaler.is_enabled() and id(self.base_optimizer) not in scaler._unscaled:      # (the caller unscales first to clip)
            scaler.unscale_(self.base_optimizer)
        # the rows first_step perturbed (its tables: the gradients, and with them the live set, may have changed since); the device decides
        tabs, out = self._pending
        self._pending = None
        for table, live, _ in tabs:
            check(lib().mfvit_sam_restore(ptr(table), table.shape[0], out.data_ptr() + 4, stream()), "mfvit_sam_restore")
            _bump_versions(live)
        ret = scaler.step(self.base_optimizer) if scaler is not None else self.base_optimizer.step()
        if zero_grad:
            self.zero_grad()
        return ret

    @torch.no_grad()
    def step(self, closure=None):
        if closure is None:
            raise RuntimeError("SAM.step() needs a closure that runs the second forward and backward pass")
        closure = torch.enable_grad()(closure)
        self.first_step(zero_grad=True)
        closure()
        return self.second_step()


# ------------------------------------------------------------------------------------------------ gradient-norm clipping
def _clip_args(optimizers, norm_type):
    if isinstance(optimizers, _TableOptimizer):
        opts = [optimizers]
    else:
        try:
            opts = list(optimizers)
        except TypeError:
            opts = None
        if not opts or not all(isinstance(o, _TableOptimizer) for o in opts):
            raise TypeError("mfvit.optim.clip_grad_norm_ / grad_norm take the optimizer(s) of mfvit.optim, not a parameter iterable: the device "
                            "chunk tables the kernels stream over live on the optimizer (for bare parameters use torch.nn.utils.clip_grad_norm_)")
    kind = {2.0: 0, float("inf"): 1}.get(float(norm_type))
    if kind is None:
        raise NotImplementedError(f"norm_type {norm_type!r}: the HIP kernels implement the L2 and the inf norm; torch.nn.utils.clip_grad_norm_ "
                                  "has the other orders")
    devs = {next(p for g in o.param_groups for p in g["params"]).device for o in opts}
    if len(devs) != 1:
        raise ValueError(f"the optimizers of one clip_grad_norm_ / grad_norm call must be on one device, got {sorted(map(str, devs))}")
    return opts, kind, devs.pop()


@torch.no_grad()
def _grad_norm(optimizers, max_norm, norm_type, error_if_nonfinite, per_tensor, scale):
    opts, kind, dev = _clip_args(optimizers, norm_type)
    h, st = lib(), stream()
    scratch = opts[0]._cache().setdefault("clip", {})      # partials of the last call (sized by row count) and joined row indices
    part = scratch.get("partials")
    tabs, rows, nt = [], 0, 0
    for o in opts:
        for gi, g in enumerate(o.param_groups):
            o._pre(gi)                                      # data parallel: this group's exchange is joined before its gradients are read
            table, n, _ = o._table(gi, g)
            if table is None:
                continue
            nrows = table.shape[0]
            if part is None or rows + nrows > part.numel():
                grown = torch.empty(max(1024, rows + nrows, 2 * (0 if part is None else part.numel())), device=dev, dtype=torch.float32)
                if rows:
                    grown[:rows].copy_(part[:rows])
                part = scratch["partials"] = grown
            check(h.mfvit_grad_norm_partials(ptr(table), nrows, kind, part.data_ptr() + 4 * rows, st), "mfvit_grad_norm_partials")
            tabs.append((table, o._cache()[gi]["row_tensor"], nt))
            rows += nrows
            nt += n
    if not tabs:
        zero = torch.zeros((), device=dev, dtype=torch.float32)
        return (zero, torch.zeros(0, device=dev, dtype=torch.float32)) if per_tensor else zero
    row_tensor = norms = None
    if per_tensor:
        norms = torch.empty(nt, device=dev, dtype=torch.float32)
        if len(tabs) == 1:
            row_tensor = tabs[0][1]
        else:       # tensor indices counted through all tables; joined once per set of tables (the cached tuple keeps them alive: ids stay unique)
            key = tuple(id(rt) for _, rt, _ in tabs)
            joined = scratch.setdefault("joined", {})
            hit = joined.get(key)
            if hit is None:
                if len(joined) >= 8:
                    joined.clear()
                hit = joined[key] = (torch.cat([rt + base for _, rt, base in tabs]), [rt for _, rt, _ in tabs])
            row_tensor = hit[0]
    out = torch.empty(2, device=dev, dtype=torch.float32)       # a fresh pair per call: the caller keeps out[0]
    check(h.mfvit_grad_clip_coef(ptr(part), ptr(row_tensor), rows, nt, kind, float(max_norm), ptr(norms), ptr(out), st), "mfvit_grad_clip_coef")
    total = out[0]
    if error_if_nonfinite and not bool(torch.isfinite(total)):      # the only host synchronisation, as in torch
        raise RuntimeError(f"The total norm of order {float(norm_type)} for gradients from `parameters` is non-finite, so it cannot be clipped. "
                           "To disable this error and scale the gradients by the non-finite norm anyway, set `error_if_nonfinite=False`")
    if scale:
        coef = out.data_ptr() + 4
        for table, _, _ in tabs:
            check(h.mfvit_grad_scale(ptr(table), table.shape[0], coef, st), "mfvit_grad_scale")
    return (total, norms) if per_tensor else total


def clip_grad_norm_(optimizers, max_norm, norm_type=2.0, error_if_nonfinite=False, per_tensor=False):
    """torch.nn.utils.clip_grad_norm_ over the chunk tables of one optimizer of this module or a sequence of them: ONE total norm over the
    gradients of every param group of every optimizer given (parameters without a gradient are skipped), then g *= min(1, max_norm / (total + 1e-6)).
    A norm pass per table (mfvit_grad_norm_partials), one finalize (mfvit_grad_clip_coef) and a scale pass per table (mfvit_grad_scale) that touches
    no memory when the coefficient is 1; every sum is taken in a fixed order, and nothing waits for the GPU unless `error_if_nonfinite` is set.
    Returns the total norm as a 0-dim f32 device tensor, with per_tensor=True (total, norms of the parameters that have gradients, in order).
    norm_type: 2 or inf.  Call it where torch's goes: after backward() - after ``scaler.unscale_(optimizer)`` with a GradScaler - and before step()."""
    return _grad_norm(optimizers, max_norm, norm_type, error_if_nonfinite, per_tensor, True)


def grad_norm(optimizers, norm_type=2.0, per_tensor=False):
    """The total gradient norm clip_grad_norm_ would return (and the per-tensor norms), for logging: the gradients are not touched."""
    return _grad_norm(optimizers, float("inf"), norm_type, False, per_tensor, False)
