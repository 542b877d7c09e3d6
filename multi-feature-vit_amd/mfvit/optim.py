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

    # ``single_launch=True`` (Adam / AdamW / SGD): step(), unscale_ and the norm and scale passes of clip_grad_norm_ / grad_norm run ONE launch
    # each over the joined table of all param groups instead of one per group - what layer-wise learning-rate decay (param_groups_layer_decay:
    # ~55 groups on the two-stream model) needs.  ``before_group(gi)`` is then called for every group, in order, BEFORE that launch: the
    # data-parallel overlap of one group's update with the next group's gradient exchange is given up in this mode.
    single_launch = False

    def _joined(self):
        """(joined table, parts) over the groups that have gradients, parts = [(gi, group, table, ntensors, live, row_tensor)]; (None, []) when
        no group has one.  The joined table is the per-group tables back to back, in group order, with the position of the group among `parts`
        - its hyper entry for mfvit_*_step_groups - in the upper half of the flag column.  Made on the device (a cat and one add; the addend goes
        up through pinned memory, nothing waits) and cached by the identities of the group tables, which the cached tuple keeps alive."""
        parts = []
        for gi, g in enumerate(self.param_groups):
            self._pre(gi)
            table, nt, live = self._table(gi, g)
            if table is not None:
                parts.append((gi, g, table, nt, live, self._cache()[gi]["row_tensor"]))
        if not parts:
            return None, parts
        cache = self._cache().setdefault("joined", {})
        key = tuple(id(p[2]) for p in parts)
        hit = cache.get(key)
        if hit is None:
            if len(cache) >= 8:
                cache.clear()
            tabs = [p[2] for p in parts]
            host = torch.tensor([k << 32 for k, t in enumerate(tabs) for _ in range(t.shape[0])], dtype=torch.int64).pin_memory()
            joined = torch.cat(tabs)
            joined[:, 6] += host.to(joined.device, non_blocking=True)
            hit = cache[key] = (joined, tabs, host)
        return hit[0], parts

    @torch.no_grad()
    def unscale_(self, inv_scale, found_inf):
        """GradScaler.unscale_: g *= inv_scale for every gradient of this optimizer; found_inf (device f32[1]) is set to 1 when a
        gradient held an inf / nan (mfvit_amp_unscale)."""
        if self.single_launch:
            joined, _ = self._joined()
            if joined is not None:
                check(lib().mfvit_amp_unscale(ptr(joined), joined.shape[0], float(inv_scale), ptr(found_inf), stream()), "mfvit_amp_unscale")
            return
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

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, single_launch=False):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.single_launch = bool(single_launch)

    def _flag(self, p, group):
        return 1 if self.decoupled else 0

    def _launch_runs(self, g, table, live, vals):
        """The launches of one param group, `vals` = the step numbers of its live parameters before the increment.  One kernel launch serves
        one step number (bias correction): normally every parameter of the group agrees and the whole table goes out in one launch; otherwise
        (a parameter whose first gradient arrived later, an unfrozen layer, a loaded torch state dict with mixed steps) the table rows - laid
        out parameter by parameter - are launched in runs of equal step."""
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

    def _bump_steps_joined(self, parts):
        """_bump_steps for every group of `parts` at once: the 'step' scalars of ALL live parameters are views of one host vector, so ~55 groups
        cost one add and one tolist() instead of one pair each.  Returns the values before the increment, group by group."""
        cache = self._cache().setdefault(("steps", "joined"), {})
        lives = [part[4] for part in parts]
        last = cache.get("lives")
        if last is not None and len(last) == len(lives) and all(a is b for a, b in zip(last, lives)):
            sts, ends = cache["sts"], cache["ends"]
        else:
            sts = [self.state[p] for live in lives for p in live]
            ends, n = [], 0
            for live in lives:
                n += len(live)
                ends.append(n)
            cache["lives"], cache["sts"], cache["ends"] = lives, sts, ends
        views = cache.get("views")
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
        return [vals[a:b] for a, b in zip([0] + ends[:-1], ends)]

    def _step_joined(self):
        """single_launch: every group's rows in one mfvit_adam_step_groups launch, each group with its own lr / betas / eps / weight decay /
        step.  The rare case - parameters of ONE group at different step numbers - falls back to the per-group launches for this call."""
        joined, parts = self._joined()
        if joined is None:
            return
        vals = self._bump_steps_joined(parts)
        if any(v.count(v[0]) != len(v) for v in vals):
            for (_, g, table, _, live, _), v in zip(parts, vals):
                self._launch_runs(g, table, live, v)
            return
        hyper = (_lib.AdamGroup * len(parts))()
        for h, (_, g, _, _, _, _), v in zip(hyper, parts, vals):
            h.lr, h.beta1, h.beta2 = float(g["lr"]), float(g["betas"][0]), float(g["betas"][1])
            h.eps, h.weight_decay = float(g["eps"]), float(g["weight_decay"])
            h.step, h.decoupled = v[0] + 1, int(self.decoupled)
        check(lib().mfvit_adam_step_groups(ptr(joined), joined.shape[0], hyper, len(parts), stream()), "mfvit_adam_step_groups")
        _bump_versions([p for part in parts for p in part[4]])

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
        if self.single_launch:
            return self._step_joined()
        for gi, g in enumerate(self.param_groups):
            self._pre(gi)
            table, nt, live = self._table(gi, g)
            if table is None:
                continue
            # per-parameter 'step' like torch.optim (f32 scalar tensors on the host)
            self._launch_runs(g, table, live, self._bump_steps(gi, live))


class AdamW(Adam):
    """torch.optim.AdamW semantics (decoupled weight decay; default 1e-2 like torch)."""
    decoupled = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, single_launch=False):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, single_launch=single_launch)


class SGD(_TableOptimizer):
    """torch.optim.SGD semantics (momentum, L2 weight decay; no dampening / nesterov).  torch initialises 'momentum_buffer' with the
    first update d; a zero buffer gives the same first step (momentum * 0 + d), so the kernel never needs the first-step case."""
    state_names = ("momentum_buffer",)

    def __init__(self, params, lr=1e-3, momentum=0, weight_decay=0, dampening=0, nesterov=False, single_launch=False):
        if dampening != 0 or nesterov:
            raise NotImplementedError("the HIP SGD kernel implements the reference's configuration (MAIN_CA:445-448): no dampening, no nesterov")
        # dampening / nesterov are kept in the group so that torch.optim.SGD can load this optimizer's state dict (and vice versa)
        super().__init__(params, dict(lr=lr, momentum=momentum, weight_decay=weight_decay, dampening=0, nesterov=False))
        self.single_launch = bool(single_launch)

    @torch.no_grad()
    def step(self):
        if self.single_launch:      # every group's rows in one mfvit_sgd_step_groups launch, each group with its own lr / momentum / weight decay
            joined, parts = self._joined()
            if joined is None:
                return
            hyper = (_lib.SgdGroup * len(parts))()
            for h, (_, g, _, _, _, _) in zip(hyper, parts):
                h.lr, h.momentum, h.weight_decay = float(g["lr"]), float(g["momentum"]), float(g["weight_decay"])
            check(lib().mfvit_sgd_step_groups(ptr(joined), joined.shape[0], hyper, len(parts), stream()), "mfvit_sgd_step_groups")
            _bump_versions([p for part in parts for p in part[4]])
            return
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
        # single_launch belongs to the base optimizer object (its step, unscale_ and clipping passes), not to the param groups; the perturb and
        # restore passes keep SAM's own per-group tables
        single = {"single_launch": True} if kwargs.pop("single_launch", False) else {}
        super().__init__(params, dict(rho=rho, adaptive=adaptive, **kwargs))
        self.base_optimizer = base_optimizer(self.param_groups, **single, **kwargs)
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
    launched = []                                           # the tables the norm pass ran over = the ones the scale pass runs over
    for o in opts:
        if o.single_launch:                                 # one launch over the joined table: the same rows in the same order, so the same partials
            table, parts = o._joined()
            if table is None:
                continue
            nrows = table.shape[0]
            if part is None or rows + nrows > part.numel():
                grown = torch.empty(max(1024, rows + nrows, 2 * (0 if part is None else part.numel())), device=dev, dtype=torch.float32)
                if rows:
                    grown[:rows].copy_(part[:rows])
                part = scratch["partials"] = grown
            check(h.mfvit_grad_norm_partials(ptr(table), nrows, kind, part.data_ptr() + 4 * rows, st), "mfvit_grad_norm_partials")
            launched.append(table)
            for _, _, gtable, n, _, rt in parts:
                tabs.append((gtable, rt, nt))
                nt += n
            rows += nrows
            continue
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
            launched.append(table)
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
        for table in launched:
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


# ------------------------------------------------------------------------------------------------ layer-wise learning-rate decay
def _layer_units(module):
    """[(name prefix, module, is an image encoder)] of `module`: the VisionTransformerMoCo encoders inside it (itself, when it is one), each
    with a layer map of its own, behind what is left of the module's own parameters."""
    from .encoder import VisionTransformerMoCo
    if isinstance(module, VisionTransformerMoCo):
        return [("", module, True)]
    vits = []
    for name, sub in module.named_modules():
        if isinstance(sub, VisionTransformerMoCo) and not any(name.startswith(v + ".") for v, _, _ in vits):
            vits.append((name, sub, True))
    return [("", module, False)] + [(n + ".", s, True) for n, s, _ in vits]


def _vit_layer_id(name, depth):
    if name in ("cls_token", "pos_embed") or name.startswith("patch_embed."):
        return 0
    if name.startswith("blocks."):
        return int(name.split(".")[1]) + 1
    return depth + 1          # norm.*, head.* and whatever else sits behind the blocks


def param_groups_layer_decay(modules, lr, weight_decay=0.05, layer_decay=0.75, no_weight_decay_list=("pos_embed", "cls_token")):
    """Param groups with layer-wise learning-rate decay (BEiT / MAE ``layer_decay``, timm's ``param_groups_layer_decay``) for Adam / AdamW / SGD.
    `modules`: a module or a sequence of modules, e.g. ``[fusion, vit_cxr, vit_enh]``.

    A VisionTransformerMoCo of depth L has L + 2 layer ids: cls_token, pos_embed and patch_embed.* are layer 0, blocks.i.* (LoRA tensors
    included) layer i + 1, norm.* and head.* layer L + 1, and layer k trains at ``lr * layer_decay ** (L + 1 - k)``.  Every other
    parameter - Fus_CrossViT's own, the projector / predictor around a base encoder - has scale 1 (layer_id None).  No weight decay for
    parameters with ndim <= 1, for *.bias and for the names of `no_weight_decay_list`; parameters with requires_grad=False are skipped.
    One group per (module, layer id, decays?) that is not empty: module by module, in ascending layer id, the decaying group first.  A
    group holds plain values - params, lr (= lr * lr_scale), lr_scale, weight_decay, layer_id, param_names - so optimizer state dicts
    pickle as before and load into torch.optim.AdamW built from the same groups.  ``mfvit.schedules.adjust_learning_rate`` multiplies by
    lr_scale; build the optimizer with ``single_launch=True``, or every group costs a launch per operation."""
    mods = [modules] if isinstance(modules, torch.nn.Module) else list(modules)
    skip = set(no_weight_decay_list)
    groups, seen = [], set()
    for module in mods:
        units = _layer_units(module)
        inner = [prefix for prefix, _, is_vit in units if is_vit and prefix]
        for prefix, unit, is_vit in units:
            depth = unit.depth if is_vit else None
            by_key = {}
            for name, p in unit.named_parameters():
                if not p.requires_grad or id(p) in seen or (not is_vit and any(name.startswith(i) for i in inner)):
                    continue
                seen.add(id(p))
                layer = _vit_layer_id(name, depth) if is_vit else None
                decays = not (p.ndim <= 1 or name.endswith(".bias") or name in skip)
                entry = by_key.setdefault((-1 if layer is None else layer, not decays), (layer, decays, [], []))
                entry[2].append(p)
                entry[3].append(prefix + name)
            for key in sorted(by_key):
                layer, decays, params, names = by_key[key]
                scale = 1.0 if layer is None else float(layer_decay) ** (depth + 1 - layer)
                groups.append({"params": params, "lr": lr * scale, "lr_scale": scale, "weight_decay": float(weight_decay) if decays else 0.0,
                               "layer_id": layer, "param_names": names})
    return groups


# ------------------------------------------------------------------------------------------------ EMA of the model weights
def _arena_of(module):
    """(flat f32 arena, the parameters that are views of it) of a module of this package; TypeError for a module without one."""
    from .arena import ParamArena
    flat_fn = getattr(module, "flat_parameters", None)
    arena = module.__dict__.get("_arena")
    if callable(flat_fn) and isinstance(arena, ParamArena):
        return flat_fn(), arena.params
    if callable(flat_fn) and module.__dict__.get("_arena_params") is not None:
        return flat_fn(), module._arena_params
    raise TypeError(f"mfvit.optim.ModelEma needs modules whose parameters live in a flat arena (flat_parameters(): the encoders, Fus_CrossViT), "
                    f"not {type(module).__name__}: the update is one mfvit_ema_update launch per arena")


_RUNTIME_ATTRS = ("_feat_cache", "_ws_pool", "_shadow", "_grad_arena", "_last_grad_arena", "_side")     # caches a copy must not share or clone


class ModelEma:
    """timm's ``ModelEmaV2``: an exponential moving average of the weights, kept for evaluation.  ``ModelEma(modules, decay=0.9998, warmup=False)``
    holds deep copies of `modules` (a module or a sequence, e.g. ``[fusion, vit_cxr, vit_enh]`` - copied together, so a copied Fus_CrossViT
    drives the copied encoders) in eval() mode with gradients off.  ``update(modules)`` goes after ``optimizer.step()``:
    ema = ema * d + w * (1 - d), one mfvit_ema_update launch per arena (and one per parameter outside it: an encoder's head), with the
    parameter versions bumped so the weight shadows follow; buffers are copied.  d = decay, or with warmup=True min(decay, (1 + t) / (10 + t)),
    t = the number of updates so far (counted on the host).  ``.modules`` / ``.module`` (the first) run the evaluation forward;
    ``state_dict()`` / ``load_state_dict()`` carry the copies' state dicts and t."""

    def __init__(self, modules, decay=0.9998, warmup=False):
        import copy
        mods = [modules] if isinstance(modules, torch.nn.Module) else list(modules)
        if not mods:
            raise ValueError("ModelEma needs at least one module")
        if not 0.0 <= float(decay) <= 1.0:
            raise ValueError(f"decay must lie in [0, 1], got {decay!r}")
        for m in mods:
            _arena_of(m)
        memo = {}
        for m in mods:          # runtime caches (workspaces, shadows, cached features with a graph behind them) are not part of a copy
            for sub in m.modules():
                for a in _RUNTIME_ATTRS:
                    v = sub.__dict__.get(a)
                    if v is not None:
                        memo[id(v)] = {} if isinstance(v, dict) else None
        self.modules = copy.deepcopy(mods, memo)
        for m in self.modules:
            m.eval()
            m.requires_grad_(False)
            for sub in m.modules():
                if callable(getattr(sub, "_flatten", None)):
                    sub._flatten()
            _arena_of(m)
        self.decay, self.warmup, self.t = float(decay), bool(warmup), 0

    @property
    def module(self):
        return self.modules[0]

    def decay_at(self, t):
        """d of the update number t (counted from 0)."""
        return min(self.decay, (1.0 + t) / (10.0 + t)) if self.warmup else self.decay

    @torch.no_grad()
    def update(self, modules):
        from .moco_ops import ema_update_
        mods = [modules] if isinstance(modules, torch.nn.Module) else list(modules)
        if len(mods) != len(self.modules):
            raise ValueError(f"ModelEma holds {len(self.modules)} modules, update() was given {len(mods)}")
        d = self.decay_at(self.t)
        for ema, live in zip(self.modules, mods):
            src, src_params = _arena_of(live)
            dst, dst_params = _arena_of(ema)
            if dst.numel() != src.numel():
                raise ValueError(f"{type(live).__name__}: the arena has {src.numel()} elements, its average {dst.numel()}")
            ema_update_(dst, src, d, dst_params)
            inside = {id(p) for p in dst_params}
            for pe, pl in zip(ema.parameters(), live.parameters()):
                if id(pe) not in inside:
                    if not (pe.is_contiguous() and pl.is_contiguous() and pe.dtype == pl.dtype == torch.float32 and pe.shape == pl.shape):
                        raise _lib.MfvitError("ModelEma: parameters outside an arena must be contiguous f32 tensors of equal shape")
                    ema_update_(pe.detach(), pl.detach(), d, (pe,))
            for be, bl in zip(ema.buffers(), live.buffers()):
                be.copy_(bl)
        self.t += 1

    def state_dict(self):
        return {"t": self.t, "decay": self.decay, "warmup": self.warmup, "modules": [m.state_dict() for m in self.modules]}

    def load_state_dict(self, sd):
        if len(sd["modules"]) != len(self.modules):
            raise ValueError(f"ModelEma holds {len(self.modules)} modules, the state dict {len(sd['modules'])}")
        for m, s in zip(self.modules, sd["modules"]):
            m.load_state_dict(s)
        self.t = int(sd["t"])
