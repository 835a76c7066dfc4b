"""numpy fp32 restatement of the Polyak average (csrc/ema.hip, svae_op_ema / svae_set_ema) and of the schedule
SequentialVAE.enable_ema describes.

The kernel is TF's ExponentialMovingAverage.apply in its assign_sub form, e' = e - omd * (e - w), with the inner
difference, the product and the outer difference each rounded to fp32 once.  numpy's float32 ufuncs round once per
call, so the three lines of update() are that contract."""
import numpy as np

F = np.float32


def update(e, w, omd):
    """e' for float32 arrays e, w and the float32 omd."""
    e, w = np.asarray(e, F), np.asarray(w, F)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.subtract(e, w, dtype=F)
        p = np.multiply(F(omd), d, dtype=F)
        return np.subtract(e, p, dtype=F)


def decay_t(decay, n, warmup=True):
    """The decay of an averaging step taken after n earlier ones (TF's num_updates rule), in Python floats."""
    decay = float(decay)
    return min(decay, (1.0 + n) / (10.0 + n)) if warmup else decay


def omd(decay, n, warmup=True, every=1):
    """float32(1 - decay_t ** every): what the engine is armed with on an averaging step."""
    return F(1.0 - decay_t(decay, n, warmup) ** int(every))


def track(e0, snapshots, n_live, decay, warmup=True, every=1, first_iteration=1, updates=0):
    """The averages after the training steps whose parameters (after the step) are ``snapshots``: step number
    first_iteration + k averages iff it is a multiple of ``every``; only [0, n_live) ever moves.  Returns
    (ema, averaging steps taken)."""
    e = np.array(e0, F, copy=True)
    n = int(updates)
    for k, w in enumerate(snapshots):
        if (first_iteration + k) % every:
            continue
        e[:n_live] = update(e[:n_live], np.asarray(w, F)[:n_live], omd(decay, n, warmup, every))
        n += 1
    return e, n
