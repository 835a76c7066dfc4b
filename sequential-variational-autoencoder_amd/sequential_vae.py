"""Drop-in mirror of the reference ``SequentialVAE`` training / test interface.

Reference interface (sequential_vae.py:1341-1391, abstract_network.py:155-160):

* ``train(input_batch, batch_target) -> float`` — one optimisation step: advances
  ``iteration``, decays the learning rate, feeds ``reg_coeff = 1 - exp(-it/5000)``,
  runs ``[train_op, loss, final_loss]`` and returns ``final_loss / H / W``.
* ``test(input_batch) -> ndarray[B,H,W,C]`` — the last training-branch MLE
  ``training_mles[-1]`` (BN in training mode, fresh eps).

Here the step runs on the HIP engine (libsvae_hip.so): the forward + backward of
the whole unrolled chain, then elementwise clip(+-10) + TF Adam on the flat
parameter buffer.  Parameters, gradients and inputs are torch device tensors whose
pointers are handed to the C ABI; no CPU fallback exists.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from .config import SVAEConfig, preset
from .weights import init_flat, param_table, unflatten


class SequentialVAE:
    def __init__(self, config="celeba", batch_size=None, device=None, seed=0, grad_hook=None, share_params_with=None,
                 averaged=False):
        """share_params_with: another SequentialVAE whose ``params`` tensor this context reads (sibling());
        the networks must agree in everything but the batch.  averaged: read that network's ``ema`` tensor
        instead (averaged())."""
        if not torch.cuda.is_available():
            raise RuntimeError("SequentialVAE (HIP engine) needs a GPU; no CPU fallback exists")
        cfg = preset(config) if isinstance(config, str) else config
        if batch_size is not None:
            cfg = preset_copy(cfg, batch=batch_size)
        self.cfg = cfg
        self.name = config if isinstance(config, str) else "custom"
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        self.batch_size = cfg.batch
        self.data_dims = [cfg.height, cfg.width, cfg.channels]
        self.iteration = 0                                 # abstract_network.py:103
        self.learning_rate = cfg.learning_rate             # sequential_vae.py:253
        self.grad_hook = grad_hook                         # e.g. data-parallel all-reduce
        self.overlap = None                                # bucketed all-reduce during backward
        self.L = _lib.lib()
        self.table, self.n_total, self.n_live = param_table(cfg)
        self._by_name = {p["name"]: p for p in self.table}
        self._owner = share_params_with
        self._siblings = {}
        self._averaged = bool(averaged)  # this context's ``params`` is its owner's ``ema`` tensor
        self._averaged_ctx = {}          # the owner's averaged() contexts, per batch
        # Polyak averaging (enable_ema): the averages [n_total] and the schedule's state
        self.ema = None
        self.ema_decay, self.ema_warmup, self.ema_every, self.ema_updates = None, True, 1, 0
        self.ema_from_checkpoint = False  # the last load_checkpoint found averages in the file
        if averaged and (share_params_with is None or share_params_with.ema is None):
            raise ValueError("an averaged context reads the averages of a network that has them (enable_ema)")
        if self._owner is not None and (preset_copy(self._owner.cfg, batch=cfg.batch) != cfg
                                        or self._owner.device != self.device):
            raise ValueError("a sibling differs from its owner in the batch only")
        with torch.cuda.device(self.device):
            self.params = (torch.from_numpy(init_flat(cfg, seed)).to(self.device) if self._owner is None
                           else self._owner.ema if averaged else self._owner.params)
            self.grads = torch.zeros(self.n_total, dtype=torch.float32, device=self.device)
            h = ctypes.c_void_p()
            c = cfg.to_c()
            _lib.check(self.L.svae_create(ctypes.byref(c), self.device.index, ctypes.byref(h)))
        self.ctx = h
        _lib.check(self.L.svae_bind(self.ctx, _lib.ptr(self.params), _lib.ptr(self.grads)), self.ctx)
        self._last_reg = 1.0
        self._forwarded = False   # a training forward has run (and no generate since): summaries() may read it
        self._summaries = None    # summaries.Summaries: plans and device buffers, built at the first call
        # Adam updates applied so far (the AdamOptimizer's step count behind beta1_power); with the
        # improvement-maximisation loss two apply_gradients run per iteration (:1267, :1306)
        self.adam_updates = 0
        self.grads_imp = None
        if cfg.add_improvement_maximization_loss:
            with torch.cuda.device(self.device):
                self.grads_imp = torch.zeros(self.n_total, dtype=torch.float32, device=self.device)
            _lib.check(self.L.svae_bind_imp(self.ctx, _lib.ptr(self.grads_imp)), self.ctx)
            pe = ctypes.c_int64()
            _lib.check(self.L.svae_imp_range(self.ctx, ctypes.byref(pe)), self.ctx)
            self.phi_end = int(pe.value)

    # ------------------------------------------------------------------ lifecycle
    def close(self):
        for a in list(getattr(self, "_averaged_ctx", {}).values()):
            a.close()
        if getattr(self, "ctx", None):
            self.L.svae_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ low level
    def _dev(self, a):
        if isinstance(a, torch.Tensor):
            t = a.to(self.device, dtype=torch.float32)
        else:
            t = torch.as_tensor(np.asarray(a, dtype=np.float32), device=self.device)
        return t.contiguous()

    def forward(self, x, target, eps=None, reg_coeff=1.0, stream=None, noise=None):
        """Forward of the unrolled chain.  eps [T,B,Dz] or None (device Philox).  With
        add_noise_to_chain, noise [T,B,H,W,C] is the N(0,1) of training_sample = mle + reg*sd*noise
        (sequential_vae.py:1090), or None (device Philox)."""
        self._sync_shared()
        x, target = self._dev(x), self._dev(target)
        nz = None
        if self.cfg.add_noise_to_chain:
            if noise is not None:
                nz = self._dev(noise)
                c = self.cfg
                if tuple(nz.shape) != (c.mc_steps, c.batch, c.height, c.width, c.channels):
                    raise ValueError("noise must be [T,B,H,W,C]")
            _lib.check(self.L.svae_set_chain_noise(self.ctx, _lib.ptr(nz)), self.ctx)
        elif noise is not None:
            raise ValueError("noise given but add_noise_to_chain is off")
        exp = (self.cfg.batch, self.cfg.height, self.cfg.width, self.cfg.channels)
        if tuple(x.shape) != exp or tuple(target.shape) != exp:
            raise ValueError("input must be %s, got %s / %s" % (exp, tuple(x.shape), tuple(target.shape)))
        e = None
        if eps is not None:
            e = self._dev(eps)
            if tuple(e.shape) != (self.cfg.mc_steps, self.cfg.batch, self.cfg.latent_dim):
                raise ValueError("eps must be [T,B,Dz]")
        self._keep = (x, target, e, nz)  # keep device inputs alive until backward
        self._last_reg = float(reg_coeff)
        _lib.check(self.L.svae_forward(self.ctx, _lib.ptr(x), _lib.ptr(target), _lib.ptr(e), float(reg_coeff),
                                       _lib.stream_ptr(stream)), self.ctx)
        self._forwarded = True

    def backward(self, stream=None):
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        with torch.cuda.stream(s):  # overlapped DP hooks enqueue on the caller's stream
            _lib.check(self.L.svae_backward(self.ctx, _lib.stream_ptr(s)), self.ctx)
        if self.overlap is not None:
            self.overlap.check()
        if self.grad_hook is not None:
            self.grad_hook(self.grads[:self.n_live])

    def enable_overlapped_allreduce(self, dist, group=None, force=False):
        """Data parallel: all-reduce the gradient in per-step buckets during the backward
        (parallel.OverlappedAllReduce) instead of one call after it."""
        from .parallel import OverlappedAllReduce
        self.overlap = OverlappedAllReduce(self, dist, group, force=force)
        return self.overlap

    def backward_apply(self, lr=None, step=None, stream=None):
        """backward() then apply_gradients() as one engine call (svae_backward_adam): every chain
        step's generator/encoder bucket gets its clip + Adam update on the engine's side stream as
        soon as the backward has finished it (after that bucket's overlapped all-reduce), the
        recognition bucket last.  Bit for bit the parameters of the two separate calls."""
        lr = self.learning_rate if lr is None else lr
        step = self._adam_step(step)
        if self.grad_hook is not None:  # the exchange follows the whole backward: Adam after it
            self.backward(stream)
            self.apply_gradients(lr, step, stream)
            return
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        if self.overlap is not None:
            self.overlap.eager = True
        try:
            with torch.cuda.stream(s):
                _lib.check(self.L.svae_backward_adam(self.ctx, float(lr), int(step), float(self.cfg.clip_grad_value),
                                                     _lib.stream_ptr(s)), self.ctx)
        finally:
            if self.overlap is not None:
                self.overlap.eager = False
        if self.overlap is not None:
            self.overlap.check()

    def backward_imp(self, stream=None):
        """d improvement_maximization_loss / d every variable into ``grads_imp``
        (sequential_vae.py:1302-1303; the optimiser reads only the recognition part)."""
        if self.grads_imp is None:
            raise RuntimeError("add_improvement_maximization_loss is off")
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        _lib.check(self.L.svae_backward_imp(self.ctx, _lib.stream_ptr(s)), self.ctx)
        if self.grad_hook is not None:
            self.grad_hook(self.grads_imp[:self.phi_end])

    def apply_imp_gradients(self, lr=None, step=None, stream=None):
        """clip + Adam of the recognition variables with ``grads_imp`` (:1304-1306)."""
        lr = self.learning_rate if lr is None else lr
        step = self._adam_step(step)
        _lib.check(self.L.svae_adam_imp(self.ctx, float(lr), int(step), float(self.cfg.clip_grad_value),
                                        _lib.stream_ptr(stream)), self.ctx)

    def imp_loss_value(self, reg_coeff=None):
        """``self.improvement_maximization_loss`` (:1189-1199) = sum_{t>=1} reg * coeff * -mean_b
        ||mle_t - mle_{t-1}||^2."""
        reg = self._last_reg if reg_coeff is None else reg_coeff
        tot = 0.0
        for t in range(1, self.cfg.mc_steps):
            tot += float(self.copy_out(_lib.BUF_IMP_IMG, t, self.cfg.batch).double().mean())
        return -reg * self.cfg.latent_pred_loss_coeff * tot

    def _adam_step(self, step):
        """The Adam step an update runs as (TF's beta1_power = 0.9^step): the next one by default.
        Every update path records it, so save_checkpoint's beta powers match the updates taken
        whichever API (train, backward_apply, apply_gradients, apply_imp_gradients) drove them."""
        step = self.adam_updates + 1 if step is None else int(step)
        self.adam_updates = step
        return step

    def apply_gradients(self, lr=None, step=None, stream=None):
        lr = self.learning_rate if lr is None else lr
        step = self._adam_step(step)
        _lib.check(self.L.svae_adam(self.ctx, float(lr), int(step), float(self.cfg.clip_grad_value),
                                    _lib.stream_ptr(stream)), self.ctx)

    def copy_out(self, which, step, n):
        out = torch.empty(n, dtype=torch.float32, device=self.device)
        _lib.check(self.L.svae_copy_out(self.ctx, which, step, _lib.ptr(out), n, _lib.stream_ptr()), self.ctx)
        return out

    def step_stats(self):
        """[T,2] tensor of (mean recon_t, mean KL_t)  (sequential_vae.py:1163-1164)."""
        return torch.stack([self.copy_out(_lib.BUF_STEP_STATS, t, 2) for t in range(self.cfg.mc_steps)])

    def loss_value(self, stats=None, reg_coeff=None):
        """``self.loss`` (sequential_vae.py:1166-1176) = mean over the batch of the per-image ELBO."""
        st = self.step_stats() if stats is None else stats
        st = st.double().cpu().numpy() if isinstance(st, torch.Tensor) else np.asarray(st, np.float64)
        reg = self._last_reg if reg_coeff is None else reg_coeff
        T = self.cfg.mc_steps
        tot = 0.0
        for t in range(T):
            c = self.cfg.first_step_loss_coeff if t == 0 else 1.0
            if self.cfg.intermediate_reconstruction or t == T - 1:
                tot += 16.0 * c * st[t, 0]
            tot += reg * c * self.cfg.kl_on(t) * st[t, 1]
        return tot

    def elbo_per_image(self):
        T, B = self.cfg.mc_steps, self.cfg.batch
        out = torch.zeros(B, dtype=torch.float64, device=self.device)
        for t in range(T):
            c = self.cfg.first_step_loss_coeff if t == 0 else 1.0
            if self.cfg.intermediate_reconstruction or t == T - 1:
                out += 16.0 * c * self.copy_out(_lib.BUF_REC_IMG, t, B).double()
            out += self._last_reg * c * self.cfg.kl_on(t) * self.copy_out(_lib.BUF_KL_IMG, t, B).double()
        return out

    def sample(self, t=-1):
        """training_samples[t] (:963): the MLE plus reg * stddevs * noise under add_noise_to_chain."""
        t = t % self.cfg.mc_steps
        c = self.cfg
        return self.copy_out(_lib.BUF_SAMPLE, t, c.batch * c.height * c.width * c.channels).view(
            c.batch, c.height, c.width, c.channels)

    def stddevs(self, t=-1):
        """Predicted stddevs [B,H,W,1] of step t (stddevs_prediction, :1866-1875)."""
        t = t % self.cfg.mc_steps
        c = self.cfg
        return self.copy_out(_lib.BUF_STDDEV, t, c.batch * c.height * c.width).view(c.batch, c.height, c.width, 1)

    def xhat(self, t=-1):
        t = t % self.cfg.mc_steps
        c = self.cfg
        return self.copy_out(_lib.BUF_XHAT, t, c.batch * c.height * c.width * c.channels).view(
            c.batch, c.height, c.width, c.channels)

    def latent(self, which, t):
        return self.copy_out(which, t, self.cfg.batch * self.cfg.latent_dim).view(self.cfg.batch, self.cfg.latent_dim)

    def summaries(self, lr=None):
        """The reference's training summaries (summaries.summary_names(cfg), in that order) as {name: float}
        from device state as it stands: the last forward's loss terms and latents, the bound gradient buffers
        as they are, the parameters as they are (after train(): the updated weights and the gradients that
        produced the update).  No forward runs, so no Philox counter moves and training is bit for bit what it
        is without the call.  Update ratios are lr * grads_norm / weights_norm (:1288), lr defaulting to
        ``learning_rate``.  Plans and device buffers are built at the first call and kept; one device -> host
        copy per call."""
        if not self._forwarded:
            raise RuntimeError("summaries() describes the last forward: run forward() or train() first")
        if self._summaries is None:
            from .summaries import Summaries
            self._summaries = Summaries(self)
        return self._summaries(self, self.learning_rate if lr is None else float(lr))

    def param_dict(self):
        return unflatten(self.params.cpu().numpy(), self.table)

    def grad_dict(self):
        return unflatten(self.grads.cpu().numpy(), self.table)

    def param(self, name):
        """Read-only copy of one variable (write through set_param, or write ``params`` and call
        params_updated(): in bf16 mode the engine keeps bf16 copies of the weights that an
        unannounced write would leave stale)."""
        p = self._by_name[name]
        return self.params[p["offset"]:p["offset"] + p["size"]].view(p["shape"]).clone()

    def set_param(self, name, value):
        p = self._by_name[name]
        self.params[p["offset"]:p["offset"] + p["size"]] = self._dev(value).reshape(-1)
        self.params_updated()

    def params_updated(self):
        """Announce a direct write to ``params`` (copy_, dist.broadcast, a checkpoint load): the
        next forward rebuilds the engine's bf16 weight copies from the fp32 master.  Gradients
        are zeroed as by svae_bind."""
        _lib.check(self.L.svae_bind(self.ctx, _lib.ptr(self.params), _lib.ptr(self.grads)), self.ctx)

    # ------------------------------------------------------------------ Polyak averaging
    def enable_ema(self, decay=0.999, warmup=True, every=1):
        """Keep an exponential moving average of the parameters (tf.train.ExponentialMovingAverage, which the
        reference applies to its PixelCNN alone, pixel_cnn/pixelvae.py:113-114): ``ema`` [n_total], a copy of
        ``params`` as they stand, updated by the engine right behind every Adam update of train() (svae_set_ema,
        csrc/ema.hip) as e -= (1 - decay_t) * (e - w).

        On a step with ``iteration % every == 0`` decay_t = min(decay, (1 + n) / (10 + n)) with n = ema_updates
        when ``warmup`` is on (TF's num_updates rule), else ``decay``; the engine gets
        float32(1 - decay_t ** every), so that ``every`` = k averages a k-th of the steps at the same horizon.
        Other steps make no launch.  Training itself is bit for bit what it is without averaging.  Only an owner
        context averages; read the averages through averaged()."""
        if self._owner is not None:
            raise RuntimeError("a sibling context only reads its owner's parameters; enable averaging on the owner")
        decay, every = float(decay), int(every)
        if not 0.0 <= decay < 1.0 or every < 1:
            raise ValueError("enable_ema needs 0 <= decay < 1 and every >= 1")
        with torch.cuda.device(self.device):
            self.ema = self.params.clone()
        self.ema_decay, self.ema_warmup, self.ema_every, self.ema_updates = decay, bool(warmup), every, 0
        for ctx in self._averaged_ctx.values():  # contexts of an earlier enable_ema read the old tensor
            ctx.close()
        self._averaged_ctx = {}
        return self.ema

    def ema_omd(self):
        """1 - decay_t ** every of an averaging step taken now (n = ema_updates), as the float32 the engine gets."""
        d = self.ema_decay
        if self.ema_warmup:
            d = min(d, (1.0 + self.ema_updates) / (10.0 + self.ema_updates))
        return float(np.float32(1.0 - d ** self.ema_every))

    def _arm_ema(self):
        """train(): arm the engine for this iteration's updates (omd on an averaging step, 0 on the others)."""
        on = self.iteration % self.ema_every == 0
        _lib.check(self.L.svae_set_ema(self.ctx, _lib.ptr(self.ema), self.ema_omd() if on else 0.0), self.ctx)
        self.ema_updates += 1 if on else 0

    def averaged(self, batch_size=None):
        """A context like sibling() (its own gradients and arena, cached per batch, default this network's batch)
        whose ``params`` is this network's ``ema`` tensor: forward, generate, test, restore and the trainer's
        reports on the averaged weights, while the training context's last forward stays what it was.  It
        announces its parameters before every forward / generate and cannot train.  Raises without
        enable_ema()."""
        owner = self if self._owner is None else self._owner
        if owner.ema is None:
            raise RuntimeError("averaging is not enabled (enable_ema)")
        bs = owner.cfg.batch if batch_size is None else int(batch_size)
        a = owner._averaged_ctx.get(bs)
        if a is None:
            a = SequentialVAE(preset_copy(owner.cfg, batch=bs), device=owner.device.index, share_params_with=owner,
                              averaged=True)
            a.name = owner.name
            owner._averaged_ctx[bs] = a
        return a

    # ------------------------------------------------------------------ reference API
    def train(self, input_batch, batch_target, eps=None, noise=None):
        """One training update; returns the final-step reconstruction loss per pixel
        (sequential_vae.py:1341-1375).  ``eps`` [T,B,Dz] and ``noise`` [T,B,H,W,C] (extensions for
        parity tests) replace the on-device N(0,1) draws of tf.random_normal (:1022, :1090).

        With the improvement-maximisation loss, train_op = tf.group(elbo_train_op,
        pred_latent_train_op) (:1316): two apply_gradients of one AdamOptimizer, both on gradients of
        the same forward.  TF leaves their order open; here the ELBO update (all variables, Adam step
        2k-1) runs first and the improvement update (recognition variables, step 2k) second, sharing
        the Adam moments, so beta1_power advances twice per iteration as in TF.

        With enable_ema() the engine is armed before the update (_arm_ema) and averages every live parameter
        once, after its last Adam update of the step.  backward_apply / apply_gradients / apply_imp_gradients
        called by hand use whatever the last train() armed."""
        if self._owner is not None:
            raise RuntimeError("a sibling context only reads its owner's parameters; train the owner")
        self.iteration += 1
        if self.ema is not None:
            self._arm_ema()
        self.learning_rate *= self.cfg.learning_rate_decay
        reg = 1.0 - math.exp(-self.iteration / self.cfg.reg_coeff_rate)
        self.forward(input_batch, batch_target, eps, reg, noise=noise)
        if self.grads_imp is None:
            self.backward_apply(self.learning_rate)
        else:
            self.backward()
            self.backward_imp()
            self.apply_gradients(self.learning_rate)
            self.apply_imp_gradients(self.learning_rate)
        final = float(self.copy_out(_lib.BUF_STEP_STATS, self.cfg.mc_steps - 1, 2)[0])
        return final / self.data_dims[0] / self.data_dims[1]

    # ------------------------------------------------------------------ checkpoint / resume
    def _adam_state(self, m=None, v=None):
        load = m is not None
        if not load:
            m = torch.empty(self.n_live, dtype=torch.float32, device=self.device)
            v = torch.empty_like(m)
        _lib.check(self.L.svae_adam_state(self.ctx, 1 if load else 0, _lib.ptr(m), _lib.ptr(v), self.n_live,
                                          _lib.stream_ptr(torch.cuda.current_stream(self.device))), self.ctx)
        return m, v

    def save_checkpoint(self, path):
        """Training state under the reference's names (tf.train.Saver, abstract_network.py:124-135):
        every variable, the Adam slots "<name>/Adam" and "<name>/Adam_1" of the tensors on the
        executed path, "beta1_power" / "beta2_power", and iteration / learning_rate as metadata
        (which the reference does not restore).  With enable_ema() also
        "<name>/ExponentialMovingAverage" of those tensors and ema_decay / ema_warmup / ema_every / ema_updates
        as metadata.  safetensors file."""
        from safetensors.torch import save_file
        m, v = self._adam_state()
        torch.cuda.synchronize(self.device)
        P, M, V = self.params.cpu(), m.cpu(), v.cpu()
        out = {}
        for p in self.table:
            a, b = p["offset"], p["offset"] + p["size"]
            out[p["name"]] = P[a:b].reshape(p["shape"]).clone()
            if b <= self.n_live:
                out[p["name"] + "/Adam"] = M[a:b].reshape(p["shape"]).clone()
                out[p["name"] + "/Adam_1"] = V[a:b].reshape(p["shape"]).clone()
        # TF's AdamOptimizer starts beta{1,2}_power at beta{1,2} and multiplies after every update,
        # so after N updates it holds beta^(N+1) (tf.train.AdamOptimizer._create_slots / _finish)
        out["beta1_power"] = torch.tensor(0.9 ** (self.adam_updates + 1), dtype=torch.float32)
        out["beta2_power"] = torch.tensor(0.999 ** (self.adam_updates + 1), dtype=torch.float32)
        rng = ctypes.c_uint64()
        _lib.check(self.L.svae_rng_offset(self.ctx, None, ctypes.byref(rng)), self.ctx)
        meta = {"iteration": str(self.iteration), "learning_rate": repr(self.learning_rate),
                "adam_updates": str(self.adam_updates), "config": self.name, "rng_offset": str(rng.value)}
        if self.ema is not None:  # TF's slot name; the variables Adam never touches have no average either
            E = self.ema.cpu()
            for p in self.table:
                a, b = p["offset"], p["offset"] + p["size"]
                if b <= self.n_live:
                    out[p["name"] + "/ExponentialMovingAverage"] = E[a:b].reshape(p["shape"]).clone()
            meta.update(ema_decay=repr(self.ema_decay), ema_warmup=str(int(self.ema_warmup)),
                        ema_every=str(self.ema_every), ema_updates=str(self.ema_updates))
        save_file(out, path, metadata=meta)

    def load_checkpoint(self, path):
        """Restore save_checkpoint's state (init_network's restore, abstract_network.py:139-152);
        every variable must be present with its shape.  A network with enable_ema() also restores the averages
        and ema_updates (the schedule stays the one enable_ema set); from a file without averages ``ema`` becomes
        the loaded parameters and ema_updates 0 (ema_from_checkpoint tells which).  A network without averaging
        ignores those keys."""
        from safetensors import safe_open
        P = self.params.cpu()
        M = torch.zeros(self.n_live, dtype=torch.float32)
        V = torch.zeros(self.n_live, dtype=torch.float32)
        E = None
        with safe_open(path, framework="pt") as f:
            meta = f.metadata() or {}
            keys = set(f.keys())
            has_ema = any(k.endswith("/ExponentialMovingAverage") for k in keys)
            if self.ema is not None and has_ema:
                E = {}
            for p in self.table:
                a, b = p["offset"], p["offset"] + p["size"]
                if p["name"] not in keys:
                    raise KeyError("checkpoint lacks %s" % p["name"])
                t = f.get_tensor(p["name"])
                if tuple(t.shape) != tuple(p["shape"]):
                    raise ValueError("%s: shape %s, expected %s" % (p["name"], tuple(t.shape), tuple(p["shape"])))
                P[a:b] = t.reshape(-1)
                if b <= self.n_live and p["name"] + "/Adam" in keys:
                    M[a:b] = f.get_tensor(p["name"] + "/Adam").reshape(-1)
                    V[a:b] = f.get_tensor(p["name"] + "/Adam_1").reshape(-1)
                if E is not None and p["name"] + "/ExponentialMovingAverage" in keys:
                    E[a] = f.get_tensor(p["name"] + "/ExponentialMovingAverage").reshape(-1)
        if E is not None:  # a variable without a stored average (the frozen tail) averages to itself
            avg = P.clone()
            for a, t in E.items():
                avg[a:a + t.numel()] = t
            E = avg
        self.params.copy_(P.to(self.device))
        if self.ema is not None:
            self.ema.copy_((P if E is None else E).to(self.device))
            self.ema_updates = int(meta.get("ema_updates", 0)) if E is not None else 0
            self.ema_from_checkpoint = E is not None
        self._adam_state(M.to(self.device), V.to(self.device))
        self.params_updated()  # caller-written parameters: rebuild the engine's bf16 copies
        torch.cuda.synchronize(self.device)
        per_it = 2 if self.grads_imp is not None else 1  # Adam updates per iteration
        if "iteration" in meta:
            self.iteration = int(meta["iteration"])
            self.adam_updates = int(meta.get("adam_updates", per_it * self.iteration))
        elif "beta1_power" in keys:  # a TF-converted checkpoint: recover the Adam step from beta1^(N+1)
            with safe_open(path, framework="pt") as f:
                b1p = float(f.get_tensor("beta1_power"))
            self.adam_updates = max(0, int(round(math.log(b1p) / math.log(0.9))) - 1)
            self.iteration = self.adam_updates // per_it
        else:
            self.iteration = 0
            self.adam_updates = 0
        self.learning_rate = float(meta.get("learning_rate", self.learning_rate))
        if "rng_offset" in meta:  # the engine's own draws (eps with none given) go on where the saved run stood
            rng = ctypes.c_uint64(int(meta["rng_offset"]))
            _lib.check(self.L.svae_rng_offset(self.ctx, ctypes.byref(rng), None), self.ctx)

    def generate(self, z=None, stream=None, noise=None):
        """Generator chain on latents z [T,B,Dz] (None: N(0,1) on device), no recognition network
        (sequential_vae.py:947-952, :1025).  With add_noise_to_chain, ``noise`` [T,B,H,W,C] injects
        the chain noise (None: drawn on device, never the last forward's).  Returns [x_hat_t]
        device tensors [B,H,W,C]."""
        self._sync_shared()
        e = None
        if z is not None:
            e = self._dev(z)
            if tuple(e.shape) != (self.cfg.mc_steps, self.cfg.batch, self.cfg.latent_dim):
                raise ValueError("z must be [T,B,Dz]")
        nz = None
        if noise is not None:
            if not self.cfg.add_noise_to_chain:
                raise ValueError("noise given but add_noise_to_chain is off")
            nz = self._dev(noise)
            _lib.check(self.L.svae_set_chain_noise(self.ctx, _lib.ptr(nz)), self.ctx)
        self._keep = (e, nz)
        self._forwarded = False  # svae_generate invalidates the training forward state summaries() reads
        _lib.check(self.L.svae_generate(self.ctx, _lib.ptr(e), _lib.stream_ptr(stream)), self.ctx)
        return [self.xhat(t) for t in range(self.cfg.mc_steps)]

    def generate_mc_samples(self, input_batch=None, batch_size=None):
        """Reference generate_mc_samples (sequential_vae.py:1393-1428, add_noise_to_chain=False):
        [x_0 ~ U[0,1) (the chain's unused initial sample, :947-949), x_hat_0, ..., x_hat_{T-1}]
        as numpy arrays; latents N(0,1).  Only the batch size the context was built for is valid."""
        bs = self.cfg.batch if batch_size is None else batch_size
        if bs != self.cfg.batch:
            raise ValueError("batch_size must equal the context batch (%d)" % self.cfg.batch)
        x0 = torch.rand(bs, self.cfg.height, self.cfg.width, self.cfg.channels, device=self.device)
        return [x0.cpu().numpy()] + [x.cpu().numpy() for x in self.generate()]

    def test(self, input_batch):
        """training_mles[-1] for the batch (sequential_vae.py:1381-1391; reg_coeff default 1.0)."""
        self.forward(input_batch, input_batch, None, 1.0)
        return self.xhat(-1).cpu().numpy()

    def restore(self, images, range=(-1.0, 1.0), stride=None, steps=-1, seed=None, known=None, as_uint8=None,
                max_bytes=4 << 30, weights="train"):
        """Apply the network to whole images of any size: overlapping tiles of the network's own h x w go through
        the chain and are blended back with a triangular window (restore.py, csrc/tiles.hip).

        ``images`` is [H,W,C] or [N,H,W,C] (C the network's), uint8 or float (floats already in ``range``), numpy
        or torch.  ``stride`` (an int or a pair, default half the tile per axis) places the tiles; the last tile
        of an axis is pulled back to the edge, nothing is padded.  An image smaller than the tile is
        edge-replicated up to it and cropped afterwards.  ``steps`` is a chain step (negative: from the end) or
        "all".  Returns a device tensor [N,H,W,C], or [T,N,H,W,C] for "all": uint8 (quantised from ``range``) if
        ``as_uint8``, which defaults to the input being uint8, else float32.

        ``known`` ([H,W] or [N,H,W], bool or uint8) marks pixels that come back exactly as given: the inpainting
        use.  It is the complement of the ``mask`` svae_op_degrade_batch writes (1 where a pixel was cut out).

        Tiles are walked in windows of the batch B as NoisyTrainer.evaluate() walks a split: first = 0, B, ...;
        with a remainder the last window is [n_tiles - B, n_tiles), of which only the rows not yet produced are
        kept; fewer than B tiles make one window that wraps around, so that a batch holds real tiles only.
        BatchNorm runs on batch statistics, so a tile's output depends on its window
        companions: the same image restored alone and among others differs slightly, and a lone tile-sized image
        fills its window with B copies of itself, which leaves the batch statistics of the FC layers without
        variance (restore several images, or a larger one, per call).  Per window: svae_op_extract_tiles into a kept input buffer,
        forward(inp, inp, eps, 1.0, noise), x_hat of the requested steps into a kept [S, n_tiles, h, w, C]
        buffer; then one svae_op_blend_tiles launch.  Above ``max_bytes`` of kept tiles a ValueError advises
        fewer images per call.

        ``seed`` = None restores with eps = 0, the posterior mean (and chain noise 0 under add_noise_to_chain):
        deterministic.  ``seed`` = k draws eps and then the chain noise of every window from one
        torch.Generator(device).manual_seed(k), as evaluate() does.  Every draw is injected, so nothing of a
        training run moves: not the parameters, the Adam state or the iteration, and not the device Philox
        counter.  Afterwards the network's last forward is the last window: summaries() reads the last forward,
        so call it before restoring.  The PixelVAE head raises as in evaluate().

        ``weights`` = "ema" restores through averaged() (the Polyak averages of enable_ema) and leaves this
        context's last forward alone."""
        if weights not in ("train", "ema"):
            raise ValueError("weights must be 'train' or 'ema', got %r" % (weights,))
        from . import restore as _restore
        return _restore.restore(self if weights == "train" else self.averaged(), images, range=range, stride=stride, steps=steps, seed=seed, known=known,
                                as_uint8=as_uint8, max_bytes=max_bytes)

    # ------------------------------------------------------------------ siblings / visualisation
    def _sync_shared(self):
        """A sibling reads parameters its owner's Adam writes behind this context's bf16 and shared-weight
        copies: every forward / generate of a sibling first announces them (params_updated)."""
        if self._owner is not None:
            self.params_updated()

    def sibling(self, batch_size):
        """A second context at another batch that shares this network's ``params`` tensor (its own
        gradients and arena): a context runs only the batch it was created for, and visualising or
        testing at another batch must see the parameters training has reached.  Cached per batch; a
        sibling does not train."""
        owner = self if self._owner is None else self._owner
        if self._averaged:  # the averaged weights at another batch
            return owner.averaged(batch_size)
        if batch_size == owner.cfg.batch:
            return owner
        s = owner._siblings.get(batch_size)
        if s is None:
            s = SequentialVAE(preset_copy(owner.cfg, batch=batch_size), device=owner.device.index,
                              share_params_with=owner)
            s.name = owner.name
            owner._siblings[batch_size] = s
        return s

    def training_mc_samples(self, input_batch):
        """Reference training_mc_samples (sequential_vae.py:1434-1455): the training branch's samples of the
        batch as numpy arrays, [sample_0 .. sample_{T-1}]; under add_noise_to_chain the MLEs come first,
        [mle_0 .. mle_{T-1}, sample_0 .. sample_{T-1}]."""
        self.forward(input_batch, input_batch, None, 1.0)
        T = self.cfg.mc_steps
        out = [self.sample(t).cpu().numpy() for t in range(T)]
        if self.cfg.add_noise_to_chain:
            out = [self.xhat(t).cpu().numpy() for t in range(T)] + out
        return out

    def visualize(self, epoch, dataset, base_dir, batch_size=10):
        """The reference's two chain pictures (sequential_vae.py:1461-1527) through a sibling context at
        ``batch_size``: a generated chain (column 0 the U[0,1) start generate_mc_samples returns, then
        x_hat_t) and a training chain (column 0 the input batch, then the samples); one row block per
        image, two under add_noise_to_chain (MLEs above samples) -- canvas.chain_canvas.  Written to
        <base_dir>/samples/{test,train}_epoch<epoch> and {test,train}_current; returns both canvases."""
        from . import canvas as cv
        net = self.sibling(batch_size)
        T, noisy = self.cfg.mc_steps, self.cfg.add_noise_to_chain
        disp = lambda a: dataset.display(np.asarray(a))
        folder = None if base_dir is None else base_dir + "/samples"
        out = []
        for which in ("test", "train"):
            if which == "test":
                z = net.generate_mc_samples(None, batch_size)
                start, mles = disp(z[0]), z[1:]
                samples = [net.sample(t).cpu().numpy() for t in range(T)] if noisy else None
            else:
                bx = dataset.rows(dataset.next_batch(batch_size)).to(self.device)
                if bx.dtype == torch.uint8:
                    lo, hi = dataset.range
                    bx = lo + bx.to(torch.float32) * ((hi - lo) / 255.0)
                z = net.training_mc_samples(bx)
                start = disp(bx.cpu().numpy())
                mles, samples = (z[:T], z[T:]) if noisy else (z, None)
            c = cv.chain_canvas(start, [disp(m) for m in mles], None if samples is None else [disp(s) for s in samples])
            if folder is not None:
                cv.save_canvas(c, folder, "%s_epoch%d" % (which, epoch))
                cv.save_canvas(c, folder, "%s_current" % which)
            out.append(c)
        return out


def preset_copy(cfg, **over):
    from dataclasses import replace
    return replace(cfg, **over)
