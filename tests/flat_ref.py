"""float64 restatement of the flat generator (generator_flat, sequential_vae.py:1880-1936) — test helper.

Composed from the oracle's tape, its conv2d_bn_lrelu, its recognition and step-0 ladder generator:
x -> z_0 -> x_0 is a VLAE (:1915-1916), every later step maps the previous (noisy) sample through
flat_conv_layers - 1 conv2d_bn_lrelu (4x4, stride 1, :1929-1930) and one sigmoid conv2d scaled to the
dataset range (:1934-1935).  Steps t >= 1 have no compute_encodings, split_latent, highway or shortcut;
their z_t is still drawn by the recognition ladder and its KL enters the loss.  Not collected by pytest.
"""
import numpy as np

from oracle import model as M
from oracle import spec as S
from oracle import tape as T


def make_cfg(base="tiny", **over):
    """The oracle's config dict of a flat-generator chain: `base` + add_noise_to_chain (every netname
    that selects generator_flat sets it, :769-793) + flat_conv_layers / flat_conv_filter_sizes (:245-247)."""
    cfg = S.make_config(base, add_noise_to_chain=True, **over)
    cfg.setdefault("flat_conv_layers", 6)
    cfg.setdefault("flat_conv_filter_sizes", None)
    return cfg


def flat_sizes(cfg):
    """flat_conv_filter_sizes (:246-247); entry flat_conv_layers is never read (:1926-1934)."""
    C = cfg["C"]
    return list(cfg.get("flat_conv_filter_sizes") or [C, 2 * C, 4 * C, 8 * C, 4 * C, 2 * C, C])


def build_params(cfg):
    """(table, struct, flat_struct): the variable table in creation order (name, shape, init, dead,
    zero_grad), the oracle's per-step struct, and per step t >= 1 the flat scope's layer names
    (theta/generative_flat_step_<t>: Conv.. + BatchNorm.., then the output Conv, :1923-1934)."""
    base, struct = S.build_params(cfg)
    nl, fs = cfg.get("flat_conv_layers", 6), flat_sizes(cfg)
    table, flat_struct = [], []
    for t in range(cfg["mc_steps"]):
        table += [p for p in base if p["name"].startswith("phi/inference_step_%d/" % t)]
        if t == 0:
            table += [p for p in base if p["name"].startswith("theta/generative_step_0/")]
            flat_struct.append(None)
            continue
        sc = S._Scope("theta/generative_flat_step_%d" % t, table)
        convs = [sc.conv_bn((4, 4, fs[l], fs[l + 1])) for l in range(nl - 1)]
        w, b = sc.add("Conv", [("weights", (4, 4, fs[nl - 1], cfg["C"]), "glorot", False),
                               ("biases", (cfg["C"],), "zeros", False)])
        flat_struct.append(dict(convs=convs, out=dict(w=w, b=b)))
    return table, struct, flat_struct


def shared_name(name, share_theta=True, share_phi=True):
    """Sharing map: one theta/generative_network_flat for every t >= 1 (:1919-1921)."""
    scope = name.split("/")[1]
    if share_theta and scope.startswith("generative_flat_step_"):
        return "theta/generative_network_flat/" + name.split("/", 2)[2]
    return S.shared_name(name, share_theta, share_phi)


def shared_table(cfg, share_theta=True, share_phi=True):
    seen, out = set(), []
    for p in build_params(cfg)[0]:
        n = shared_name(p["name"], share_theta, share_phi)
        if n not in seen:
            seen.add(n)
            out.append(dict(p, name=n))
    return out


def sum_shared_grads(grads, share_theta=True, share_phi=True):
    out = {}
    for n, g in grads.items():
        k = shared_name(n, share_theta, share_phi)
        out[k] = out[k] + g if k in out else np.array(g, copy=True)
    return out


def init_params(cfg, seed=0):
    from oracle.weightgen import generate
    table, struct, flat_struct = build_params(cfg)
    params = {p["name"]: generate(p["name"], p["shape"], p["init"], seed).astype(np.float64) for p in table}
    return table, struct, flat_struct, params


def generator_flat(tp, P, cfg, fst, xprev):
    """:1927-1935."""
    h = xprev
    for lay in fst["convs"]:
        h = M._conv_bn_act(tp, P, h, lay, 1, "lrelu")
    o = T.conv2d(tp, h, P[fst["out"]["w"]], 1)
    o = T.sigmoid(tp, T.bias_add(tp, o, P[fst["out"]["b"]]))
    lo, hi = cfg["range"]
    return T.affine(tp, o, hi - lo, lo)


def forward_backward_flat(cfg, struct, flat_struct, params, x, target, eps, reg=1.0, noise=None, want_grads=True):
    """loss, per-step recon / KL, xhat, sample, elbo_img, grads and dz of one training iteration
    (the loss assembly of oracle.model.forward_backward, :1146-1176)."""
    tp = T.Tape()
    P = {k: tp.leaf(v) for k, v in params.items()}
    xin = tp.leaf(np.asarray(x, np.float64))
    target = np.asarray(target, np.float64)
    Tn = cfg["mc_steps"]
    terms, coeffs, znodes = [], [], []
    out = dict(recon=[], kl=[], recon_img=[], kl_img=[], xhat=[], sample=[], z=[])
    prev = None
    for t in range(Tn):
        mu, sig = M.inference_ladder(tp, P, cfg, struct[t]["inference"], xin)
        z = T.add(tp, mu, T.mul(tp, sig, tp.leaf(np.asarray(eps[t], np.float64))))
        if t == 0:
            xhat = M.generator_ladder(tp, P, cfg, struct[0]["generator"], None, z, None)
        else:
            xhat = generator_flat(tp, P, cfg, flat_struct[t], prev)
        sample = T.add_scaled_noise(tp, xhat, cfg["noise_stddevs"][t], np.asarray(noise[t], np.float64), reg)
        rec = T.mean_sq_err_per_row(tp, xhat, target)
        kl = T.kl_per_row(tp, mu, sig, cfg["latent_prior_stddev"])
        rec_m, kl_m = T.mean_all(tp, rec), T.mean_all(tp, kl)
        c_first = cfg["first_step_loss_coeff"] if t == 0 else 1.0
        if cfg["intermediate_reconstruction"] or t == Tn - 1:
            terms.append(rec_m)
            coeffs.append(16.0 * c_first)
        terms.append(kl_m)
        coeffs.append(reg * c_first * S.kl_on(cfg, t))
        out["recon"].append(float(rec_m.v))
        out["kl"].append(float(kl_m.v))
        out["recon_img"].append(rec.v.copy())
        out["kl_img"].append(kl.v.copy())
        out["xhat"].append(xhat.v.copy())
        out["sample"].append(sample.v.copy())
        out["z"].append(z.v.copy())
        znodes.append(z)
        prev = sample
    loss = T.scalar_sum(tp, terms, coeffs)
    out["loss"] = float(loss.v)
    elbo = np.zeros(np.asarray(x).shape[0])
    for t in range(Tn):
        c_first = cfg["first_step_loss_coeff"] if t == 0 else 1.0
        if cfg["intermediate_reconstruction"] or t == Tn - 1:
            elbo += 16.0 * c_first * out["recon_img"][t]
        elbo += reg * c_first * S.kl_on(cfg, t) * out["kl_img"][t]
    out["elbo_img"] = elbo
    if want_grads:
        tp.backward(loss)
        out["grads"] = {k: (n.g if n.g is not None else np.zeros_like(n.v)) for k, n in P.items()}
        # d loss / d z_t through the generator (the KL term depends on mu, sigma, not on the draw): zero for t >= 1
        out["dz"] = [(n.g.copy() if n.g is not None else np.zeros_like(n.v)) for n in znodes]
    return out


def kl_term_grads(cfg, struct, params, x, reg, t):
    """Gradient of step t's KL term alone, reg * c_first * kl_on * mean_b KL_t (:1154-1176): what the
    recognition ladder of a flat step t >= 1 receives, since nothing in the generator reads z_t."""
    tp = T.Tape()
    P = {k: tp.leaf(v) for k, v in params.items()}
    mu, sig = M.inference_ladder(tp, P, cfg, struct[t]["inference"], tp.leaf(np.asarray(x, np.float64)))
    kl_m = T.mean_all(tp, T.kl_per_row(tp, mu, sig, cfg["latent_prior_stddev"]))
    c_first = cfg["first_step_loss_coeff"] if t == 0 else 1.0
    tp.backward(T.scalar_sum(tp, [kl_m], [reg * c_first * S.kl_on(cfg, t)]))
    return {k: (n.g if n.g is not None else np.zeros_like(n.v)) for k, n in P.items()}


def generate_flat(cfg, struct, flat_struct, params, z, noise, reg=1.0):
    """Generative mode (:947-952, :1070-1073): ladder step 0 on z_0, flat steps on the noisy samples."""
    tp = T.Tape()
    P = {k: tp.leaf(v) for k, v in params.items()}
    outs, prev = [], None
    for t in range(cfg["mc_steps"]):
        if t == 0:
            xhat = M.generator_ladder(tp, P, cfg, struct[0]["generator"], None,
                                      tp.leaf(np.asarray(z[0], np.float64)), None)
        else:
            xhat = generator_flat(tp, P, cfg, flat_struct[t], prev)
        outs.append(xhat.v.copy())
        prev = T.add_scaled_noise(tp, xhat, cfg["noise_stddevs"][t], np.asarray(noise[t], np.float64), reg)
    return outs
