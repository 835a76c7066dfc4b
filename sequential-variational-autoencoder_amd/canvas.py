"""Image canvases of the trainer and of SequentialVAE.visualize (host numpy; no GPU needed).

Images are [H, W, C] arrays already mapped to [0, 1] (DeviceDataset.display).  A canvas is [rows, cols, C].

reconstruction_canvas (the layout of the reference's NoisyTrainer.plot_reconstruction, trainer.py:158-179):
    one row block of H rows per image; three cells per block along the columns, original | noisy |
    reconstruction, separated by `border` columns.  The canvas starts white for RGB and black for one
    channel, so that is the border's colour.

chain_canvas (SequentialVAE.visualize): one row block per image, one column of W per chain position.
    Without chain noise cell (b, k) is columns[k][b].  With chain noise (two lists, MLEs and samples,
    behind a start column) image b owns two row blocks: the upper holds start | MLE_0 .. MLE_{T-1}, the
    lower holds (black) | sample_0 .. sample_{T-1}.  The canvas is black where nothing is written.
    This is not a transcription of the reference's loop: for a generated chain that loop addresses
    column t + 1 of a canvas that has len(z) columns (sequential_vae.py:1490-1500), one past the end.
"""
import os

import numpy as np


def reconstruction_canvas(original, noisy, reconstruction, num_plot=3, border=10):
    original, noisy, reconstruction = [np.asarray(a, dtype=np.float64) for a in (original, noisy, reconstruction)]
    n = min(num_plot, original.shape[0])
    H, W, C = original.shape[1:]
    fill = np.zeros if C == 1 else np.ones
    canvas = fill((n * H, 3 * W + 2 * border, C))
    for b in range(n):
        for k, img in enumerate((original, noisy, reconstruction)):
            c0 = k * (W + border)
            canvas[b * H:(b + 1) * H, c0:c0 + W] = img[b]
    return canvas


def chain_canvas(start, mles, samples=None):
    """start [B,H,W,C]; mles a list of T such arrays; samples (chain noise) a second list of T."""
    start = np.asarray(start, dtype=np.float64)
    B, H, W, C = start.shape
    T = len(mles)
    per = 1 if samples is None else 2
    canvas = np.zeros((per * B * H, (T + 1) * W, C))
    for b in range(B):
        r0 = per * b * H
        canvas[r0:r0 + H, :W] = start[b]
        for t in range(T):
            canvas[r0:r0 + H, (t + 1) * W:(t + 2) * W] = np.asarray(mles[t])[b]
            if samples is not None:
                canvas[r0 + H:r0 + 2 * H, (t + 1) * W:(t + 2) * W] = np.asarray(samples[t])[b]
    return canvas


def save_canvas(canvas, folder, stem):
    """<folder>/<stem>.png when PIL imports, else <stem>.npy (the float canvas); returns the path."""
    os.makedirs(folder, exist_ok=True)
    try:
        from PIL import Image
    except ImportError:
        path = os.path.join(folder, stem + ".npy")
        np.save(path, canvas)
        return path
    u8 = (np.clip(canvas, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)
    path = os.path.join(folder, stem + ".png")
    Image.fromarray(u8[:, :, 0] if u8.shape[-1] == 1 else u8).save(path)
    return path
