"""Drop-in handle for smplifyx/optimizers/lbfgs_ls.py's LBFGS (strong-Wolfe).  The algorithm
itself -- two-loop recursion over the last history_size pairs, first-step scaling min(1, 1/|g|_1) * lr, bracket
and zoom phases of the strong-Wolfe search, all stopping rules -- runs on the GPU in
csrc/lbfgs_body.h (specification: oracle/lbfgs_machine.py).  This object carries the hyper-
parameters and forwards `.step(closure)` to the engine batch bound to the closure.

With any other callable -- a closure the caller wrote on torch tensors, as the reference's LBFGS takes it (lbfgs_ls.py:256-445:
it zeroes the gradients, calls backward and returns the loss) -- `.step` runs the same device state machine on the caller's
evaluations (engine.BatchOptimizer, csrc/opt_ext.hip): after every evaluation the next trial point is written into the parameters.
`per_sample=True` makes every row of the parameters' leading dimension a problem of its own, with its own line search.
`wide=True` lifts the device optimiser's limits of 192 elements and 12 tensors per problem to 32768 and 256 (engine.WideOptimizer,
csrc/opt_wide.hip: one workgroup per problem instead of one wavefront); a problem within the narrow limits takes the narrow path
with unchanged bits either way."""

EXT_NVAR_MAX = 192      # SFX_NVAR_MAX: variables per problem of the device optimiser
EXT_MAX_TENSORS = 12    # SFX_MAX_GROUPS
WIDE_NVAR_MAX = 32768   # SFX_WIDE_NMAX: with wide=True
WIDE_MAX_TENSORS = 256  # SFX_WIDE_MAX_GROUPS


class LBFGS(object):
    def __init__(self, params, lr=1, max_iter=20, max_eval=None, tolerance_grad=1e-5, tolerance_change=1e-9,
                 history_size=100, line_search_fn=None, per_sample=False, poll_every=1, wide=False):
        if line_search_fn != "strong_Wolfe":
            raise RuntimeError("only 'strong_Wolfe' is supported")
        if history_size > 400 or history_size < 1:
            raise NotImplementedError("history_size must be 1..400 (the device keeps the alphas of the two-loop recursion in LDS)")
        self._params = list(params)
        self.lr, self.max_iter = lr, max_iter
        self.max_eval = max_iter * 5 // 4 if max_eval is None else max_eval
        self.tolerance_grad, self.tolerance_change, self.history_size = tolerance_grad, tolerance_change, history_size
        self.param_groups = [dict(params=self._params, lr=lr, max_iter=max_iter, max_eval=self.max_eval,
                                  tolerance_grad=tolerance_grad, tolerance_change=tolerance_change,
                                  history_size=history_size, line_search_fn=line_search_fn)]
        self._closure = None
        # a caller-written closure (see the module's docstring).  per_sample: every parameter is [B][...] and the closure returns
        # the [B] losses after loss.sum().backward().  poll_every = k: the count of running problems -- the loop's only host
        # synchronisation -- is read after every k-th evaluation; the evaluations in between that nobody needed are ignored
        self.per_sample, self.poll_every = bool(per_sample), max(1, int(poll_every))
        self._ext, self._ext_key = None, None
        self.wide = bool(wide)

    def _bind(self, engine_closure):
        self._closure = engine_closure

    def zero_grad(self, set_to_none=True):
        for p in self._params:
            p.grad = None

    def step(self, closure):
        """One optimisation step (up to max_iter L-BFGS iterations / max_eval evaluations) on
        device; returns the loss at entry, like the reference."""
        from ..fitting import EngineClosure
        c = closure if isinstance(closure, EngineClosure) else self._closure
        if c is None:
            if not callable(closure):
                raise TypeError("LBFGS.step needs a callable: a closure made by FittingMonitor.create_fitting_closure, or any "
                                "function that zeroes the gradients, calls backward and returns the loss")
            return self._step_ext(closure)
        c._check_params(self._params)
        return c.step(stage=getattr(c, "_fb_stage", None) or 0)

    # ---- a closure the caller wrote: the device state machine over the caller's evaluations --------------------------------
    def _ext_layout(self):
        """(B, lengths per problem of the parameter tensors) after the checks that need no device."""
        import torch
        ps = self._params
        if not ps:
            raise ValueError("LBFGS: no parameters")
        nvar_max, max_tensors = (WIDE_NVAR_MAX, WIDE_MAX_TENSORS) if self.wide else (EXT_NVAR_MAX, EXT_MAX_TENSORS)
        hint = "" if self.wide else "; LBFGS(..., wide=True) takes up to %d elements in up to %d tensors" % (WIDE_NVAR_MAX, WIDE_MAX_TENSORS)
        if len(ps) > max_tensors:
            raise ValueError("LBFGS.step with a caller-written closure: %d parameter tensors, the device optimiser takes at "
                             "most %d (concatenate some)%s" % (len(ps), max_tensors, hint))
        for i, p in enumerate(ps):
            if not torch.is_tensor(p):
                raise TypeError("LBFGS: parameter %d is a %s, not a tensor" % (i, type(p).__name__))
        B = 1
        if self.per_sample:
            if any(p.dim() < 1 for p in ps) or len(set(int(p.shape[0]) for p in ps)) != 1:
                raise ValueError("LBFGS(per_sample=True): every parameter needs the same leading dimension B, got shapes %s"
                                 % [tuple(p.shape) for p in ps])
            B = int(ps[0].shape[0])
            if B < 1:
                raise ValueError("LBFGS(per_sample=True): empty batch")
        lens = [p.numel() // B for p in ps]
        if sum(lens) > nvar_max or min(lens) < 1:
            shown = lens if len(lens) <= 16 else lens[:16] + ["..."]
            raise ValueError("LBFGS.step with a caller-written closure: %d elements%s in tensors of %s, the device optimiser "
                             "takes 1..%d with no empty tensor%s" % (sum(lens), " per sample" if self.per_sample else "", shown, nvar_max, hint))
        for i, p in enumerate(ps):
            if p.device.type != "cuda":
                raise ValueError("LBFGS.step with a caller-written closure: parameter %d is on %s; the optimiser runs on the GPU "
                                 "(no CPU fallback)" % (i, p.device))
            if p.dtype != torch.float32:
                raise ValueError("LBFGS.step with a caller-written closure: parameter %d is %s; float32 is needed" % (i, p.dtype))
        if len(set(p.device for p in ps)) != 1:
            raise ValueError("LBFGS: parameters on several devices: %s" % sorted(set(str(p.device) for p in ps)))
        return B, lens

    def _step_ext(self, closure):
        import torch
        from .. import engine
        B, lens = self._ext_layout()
        ps, N = self._params, sum(lens)
        dev = ps[0].device
        key = (B, tuple(lens), dev)
        resume = self._ext is not None and self._ext_key == key
        with torch.cuda.device(dev):
            if not resume:
                if self._ext is not None:
                    self._ext.close()
                # (run_fitting's own rules -- maxiters, ftol, gtol -- play no part in ONE step)
                # (within the narrow limits a wide optimiser takes the narrow path: the same bits as without the flag)
                narrow = N <= EXT_NVAR_MAX and len(lens) <= EXT_MAX_TENSORS
                handle = engine.BatchOptimizer if narrow else engine.WideOptimizer
                self._ext = handle(B, N, groups=lens, maxiters=1, ftol=0.0, gtol=0.0, lr=self.lr, max_iter=self.max_iter,
                                   max_eval=self.max_eval, history_size=self.history_size,
                                   tolerance_grad=self.tolerance_grad, tolerance_change=self.tolerance_change)
                self._ext_key = key
            opt = self._ext
            flat = lambda ts: torch.cat([t.detach().reshape(B, -1) for t in ts], 1).contiguous()

            def scatter(src, to_grad=False):
                o = 0
                with torch.no_grad():
                    for p, n in zip(ps, lens):
                        v = src[:, o:o + n].reshape(p.shape)
                        if to_grad:
                            p.grad = v.clone()
                        else:
                            p.copy_(v)
                        o += n

            xt = opt.begin(flat(ps), mode="step", resume=resume)
            n_eval = 0
            while True:
                scatter(xt)
                with torch.enable_grad():
                    loss = closure()
                if not torch.is_tensor(loss) or loss.numel() != B:
                    raise ValueError("the closure must return %s, got %s" % (
                        "the [%d] per-sample losses" % B if self.per_sample else "the loss as a one-element tensor",
                        tuple(loss.shape) if torch.is_tensor(loss) else type(loss).__name__))
                grads = [p.grad if p.grad is not None else torch.zeros_like(p) for p in ps]
                opt.tell(loss.detach().to(dev, torch.float32).reshape(B).contiguous(), flat(grads).to(torch.float32))
                n_eval += 1
                if n_eval % self.poll_every == 0 and opt.active() == 0:
                    break
            r = opt.result()
            scatter(r["x"])                      # the accepted point
            scatter(r["grad"], to_grad=True)     # the gradient of the last evaluation the step consumed (var.grad after step())
            entry = torch.as_tensor(r["result"]).to(dev)
        return entry if self.per_sample else entry.reshape(())
