"""The reference's training summaries (sequential_vae.py:968-978, 1201-1208, 1278-1314) from device state.

Every reduction over a tensor is one svae_op_tensor_stats launch pair (csrc/stats.hip): the parameter table's
tensors are the segments of one plan over ``params`` (no clamp), ``grads`` (clamp = clip_grad_value, the
value clipping the optimiser applies before tf.global_norm, :1275, :1285) and, with the improvement loss,
``grads_imp``; the latent means and stddevs of all T steps are copied into one [2][T][B Dz] buffer and reduced
by two calls over a T-segment plan, the means with clamp = latent_mean_clip (SVAE_BUF_MU is the raw mean, the
reference summarises the clipped one, :1593, :1608) and the stddevs with none.  The per-step loss terms and
the improvement terms are copied next to the statistics, so one device -> host copy brings everything.

Names are the reference's; the engine's own additions carry the prefix ``debug/``.  Not provided:
``resnet_gate_weight_step_<t>`` (:1075, the engine keeps no buffer of the highway ratio) and
``classic_reconstruction_loss_step_<t>`` (:1148, under predict_generator_noise the engine keeps the NLL only).
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib

COLS = 8
C_FINITE, C_SUM, C_ABS, C_SQ, C_MAX, C_CLIPPED, C_NONFINITE = range(7)
GROUPS = ("theta", "phi")  # TF's test: the substring in the variable name (:1228)


def summary_names(cfg):
    """The ordered scalar names ``SequentialVAE.summaries()`` returns for a configuration (pure Python)."""
    T = cfg.mc_steps
    imp = bool(cfg.add_improvement_maximization_loss)
    names = ["loss"]
    for t in range(T):
        names += ["reconstruction_loss_step_%d" % t, "regularization_loss_step_%d" % t,
                  "latent_mean_avg_magnitude_step_%d" % t, "latent_mean_avg_step_%d" % t,
                  "latent_stddev_avg_step_%d" % t, "training_stddev_avg_magnitude_step_%d" % t]
        if imp and t >= 1:
            names.append("improvement_maximization_loss_step_%d" % t)
    names += ["theta_weights_norm", "phi_weights_norm", "theta_elbo_grads_norm", "phi_elbo_grads_norm",
              "theta_elbo_update_ratio", "phi_elbo_update_ratio"]
    if imp:
        names += ["phi_latent_pred_grads_norm", "phi_latent_pred_update_ratio"]
    names += ["debug/theta_grads_clipped_fraction", "debug/phi_grads_clipped_fraction",
              "debug/theta_grads_max_abs", "debug/phi_grads_max_abs", "debug/grads_nonfinite",
              "debug/weights_nonfinite"]
    return names


def stats_plan(offsets, lengths):
    """(table, n_chunks) of svae_op_stats_plan for host lists of segment offsets and lengths: the int64 table
    as a numpy array (layout: include/svae_hip.h).  Needs the library, not a GPU."""
    L = _lib.lib()
    n = len(offsets)
    i64p = ctypes.POINTER(ctypes.c_int64)
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    ln = np.ascontiguousarray(lengths, dtype=np.int64)
    args = (off.ctypes.data_as(i64p), ln.ctypes.data_as(i64p), n)
    nc = L.svae_op_stats_plan(*args, None, 0)
    if nc < 0:
        _lib.check(nc)
    table = np.zeros(n + 1 + 2 * nc, dtype=np.int64)
    got = L.svae_op_stats_plan(*args, table.ctypes.data_as(i64p), table.size)
    if got < 0:
        _lib.check(got)
    assert got == nc
    return table, int(nc)


class _Plan:
    """A plan on the device: built once per (array, segmentation) and reused."""

    def __init__(self, offsets, lengths, device):
        table, self.n_chunks = stats_plan(offsets, lengths)
        self.n_seg = len(offsets)
        self.table = torch.from_numpy(table).to(device)


class Summaries:
    """Plans and device buffers of one network's summaries (kept by SequentialVAE after the first call)."""

    def __init__(self, net):
        cfg, dev = net.cfg, net.device
        T, B = cfg.mc_steps, cfg.batch
        tab = sorted(net.table, key=lambda p: p["offset"])
        self.group = {g: np.array([g in p["name"] for p in tab]) for g in GROUPS}
        self.imp = net.grads_imp is not None
        self.pgn = bool(cfg.predict_generator_noise)
        with torch.cuda.device(dev):
            self.p_table = _Plan([p["offset"] for p in tab], [p["size"] for p in tab], dev)
            nl = B * cfg.latent_dim
            self.p_lat = _Plan([t * nl for t in range(T)], [nl] * T, dev)
            self.lat = torch.empty(2, T, nl, dtype=torch.float32, device=dev)
            plans = [self.p_table, self.p_lat]
            if self.pgn:
                ns = B * cfg.height * cfg.width
                self.p_sd = _Plan([t * ns for t in range(T)], [ns] * T, dev)
                self.sd = torch.empty(T, ns, dtype=torch.float32, device=dev)
                plans.append(self.p_sd)
            nt = self.p_table.n_seg
            # rows of the result: params, grads, [grads_imp], mu, sigma, [stddev]; then the fp32 tail:
            # step stats [T][2] and, with the improvement loss, imp_img [T][B] (row 0 unused)
            self.r_params, self.r_grads = 0, nt
            self.r_imp = 2 * nt
            self.r_mu = (3 if self.imp else 2) * nt
            self.r_sig = self.r_mu + T
            self.r_sd = self.r_sig + T
            self.rows = self.r_sd + (T if self.pgn else 0)
            self.tail_floats = 2 * T + (T * B if self.imp else 0)
            self.res = torch.zeros(self.rows * COLS + (self.tail_floats + 1) // 2, dtype=torch.float64, device=dev)
            self.tail = self.res[self.rows * COLS:].view(torch.float32)
            self.partials = torch.empty(max(1, max(p.n_chunks for p in plans)) * COLS, dtype=torch.float64,
                                        device=dev)

    def _stats(self, x, plan, c, row, s):
        _lib.check(_lib.lib().svae_op_tensor_stats(_lib.ptr(x), _lib.ptr(plan.table), plan.n_seg, plan.n_chunks,
                                                   float(c), _lib.ptr(self.partials),
                                                   _lib.ptr(self.res[row * COLS:]), s))

    def _copy(self, net, which, t, dst, s):
        _lib.check(_lib.lib().svae_copy_out(net.ctx, which, t, _lib.ptr(dst), dst.numel(), s), net.ctx)

    def enqueue(self, net):
        """Every launch and device copy of one summary, on the current stream; no synchronisation."""
        cfg = net.cfg
        T, B = cfg.mc_steps, cfg.batch
        with torch.cuda.device(net.device):
            s = _lib.stream_ptr(torch.cuda.current_stream(net.device))
            self._stats(net.params, self.p_table, math.inf, self.r_params, s)
            self._stats(net.grads, self.p_table, cfg.clip_grad_value, self.r_grads, s)
            if self.imp:
                self._stats(net.grads_imp, self.p_table, cfg.clip_grad_value, self.r_imp, s)
            for t in range(T):
                self._copy(net, _lib.BUF_MU, t, self.lat[0, t], s)
                self._copy(net, _lib.BUF_SIGMA, t, self.lat[1, t], s)
            self._stats(self.lat[0], self.p_lat, cfg.latent_mean_clip, self.r_mu, s)
            self._stats(self.lat[1], self.p_lat, math.inf, self.r_sig, s)
            if self.pgn:
                for t in range(T):
                    self._copy(net, _lib.BUF_STDDEV, t, self.sd[t], s)
                self._stats(self.sd, self.p_sd, math.inf, self.r_sd, s)
            for t in range(T):
                self._copy(net, _lib.BUF_STEP_STATS, t, self.tail[2 * t:2 * t + 2], s)
            if self.imp:
                for t in range(1, T):
                    self._copy(net, _lib.BUF_IMP_IMG, t, self.tail[2 * T + t * B:2 * T + (t + 1) * B], s)

    def __call__(self, net, lr):
        cfg = net.cfg
        T, B = cfg.mc_steps, cfg.batch
        self.enqueue(net)
        host = self.res.cpu()  # the one device -> host copy (it waits for the stream)
        st = host[:self.rows * COLS].numpy().reshape(self.rows, COLS)
        tail = host[self.rows * COLS:].view(torch.float32).numpy().astype(np.float64)
        steps = tail[:2 * T].reshape(T, 2)
        nt = self.p_table.n_seg
        P, G = st[self.r_params:self.r_params + nt], st[self.r_grads:self.r_grads + nt]
        mu, sig = st[self.r_mu:self.r_mu + T], st[self.r_sig:self.r_sig + T]
        nl = float(B * cfg.latent_dim)
        noise = cfg.noise_list()
        reg = net._last_reg
        out = {"loss": float(net.loss_value(stats=steps))}
        for t in range(T):
            regularized = cfg.regularized_steps is None or t in cfg.regularized_steps
            out["reconstruction_loss_step_%d" % t] = float(steps[t, 0])
            # the reference's term is the constant 0 on a step outside regularized_steps (:1153-1154)
            out["regularization_loss_step_%d" % t] = float(steps[t, 1]) if regularized else 0.0
            out["latent_mean_avg_magnitude_step_%d" % t] = mu[t, C_ABS] / nl
            out["latent_mean_avg_step_%d" % t] = mu[t, C_SUM] / nl
            out["latent_stddev_avg_step_%d" % t] = sig[t, C_SUM] / nl
            if self.pgn:
                sd = st[self.r_sd + t, C_ABS] / float(B * cfg.height * cfg.width)
            else:
                sd = abs(noise[t]) if cfg.add_noise_to_chain else 0.0
            out["training_stddev_avg_magnitude_step_%d" % t] = sd
            if self.imp and t >= 1:
                img = tail[2 * T + t * B:2 * T + (t + 1) * B]
                out["improvement_maximization_loss_step_%d" % t] = -reg * cfg.latent_pred_loss_coeff * float(img.mean())
        norm = lambda rows, g: math.sqrt(float(rows[self.group[g], C_SQ].sum()))
        wn = {g: norm(P, g) for g in GROUPS}
        gn = {g: norm(G, g) for g in GROUPS}
        ratio = lambda a, b: lr * a / b if b > 0.0 else math.inf if a > 0.0 else 0.0
        for g in GROUPS:
            out["%s_weights_norm" % g] = wn[g]
        for g in GROUPS:
            out["%s_elbo_grads_norm" % g] = gn[g]
        for g in GROUPS:
            out["%s_elbo_update_ratio" % g] = ratio(gn[g], wn[g])
        if self.imp:
            pn = norm(st[self.r_imp:self.r_imp + nt], "phi")
            out["phi_latent_pred_grads_norm"] = pn
            out["phi_latent_pred_update_ratio"] = ratio(pn, wn["phi"])
        for g in GROUPS:
            fin = float(G[self.group[g], C_FINITE].sum())
            out["debug/%s_grads_clipped_fraction" % g] = float(G[self.group[g], C_CLIPPED].sum()) / fin if fin else 0.0
        for g in GROUPS:
            out["debug/%s_grads_max_abs" % g] = float(G[self.group[g], C_MAX].max()) if self.group[g].any() else 0.0
        out["debug/grads_nonfinite"] = float(G[:, C_NONFINITE].sum())
        out["debug/weights_nonfinite"] = float(P[:, C_NONFINITE].sum())
        names = summary_names(cfg)
        assert set(names) == set(out), sorted(set(names) ^ set(out))
        return {k: float(out[k]) for k in names}

