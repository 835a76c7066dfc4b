"""Whole-image restoration: images of any size go through the chain as overlapping tiles of the network's own
h x w and come back blended, masked and re-quantised (csrc/tiles.hip; the contract is in include/svae_hip.h).

``TileGrid`` is the geometry (pure Python / numpy, no GPU), ``extract_tiles`` and ``blend_tiles`` are the two ops
on the current stream, ``restore`` is what ``SequentialVAE.restore`` runs.
"""
import numpy as np
import torch

from . import _lib


def tile_count(L, t, s):
    """Tiles of extent t at stride s along an axis of extent L: ceil((L - t) / s) + 1."""
    if not 1 <= s <= t <= L:
        raise ValueError("need 1 <= stride <= tile <= extent, got stride %d, tile %d, extent %d" % (s, t, L))
    return (L - t + s - 1) // s + 1


class TileGrid:
    """Overlapping tiles of th x tw at strides (sy, sx) over nimg images of H x W x C.

    Per axis k = ceil((L - t) / s) + 1 tiles, tile i at min(i s, L - t): the last tile is pulled back to the edge,
    so nothing is padded.  ``oy`` / ``ox`` are the origins, ``w1y`` / ``w1x`` the window weights
    w1(p) = min(p + 1, t - p); tile pixel (p, q) weighs w1y[p] * w1x[q].  Tile (m, i, j) has id
    (m ky + i) kx + j (``tile_id``), ``n_tiles`` = nimg ky kx."""

    def __init__(self, nimg, H, W, C, th, tw, sy, sx):
        self.nimg, self.H, self.W, self.C = int(nimg), int(H), int(W), int(C)
        self.th, self.tw, self.sy, self.sx = int(th), int(tw), int(sy), int(sx)
        if self.nimg <= 0 or self.C <= 0:
            raise ValueError("nimg and C must be positive")
        self.ky, self.kx = tile_count(self.H, self.th, self.sy), tile_count(self.W, self.tw, self.sx)
        self.n_tiles = self.nimg * self.ky * self.kx
        self.oy = np.minimum(np.arange(self.ky) * self.sy, self.H - self.th)
        self.ox = np.minimum(np.arange(self.kx) * self.sx, self.W - self.tw)
        self.w1y = np.minimum(np.arange(self.th) + 1, self.th - np.arange(self.th))
        self.w1x = np.minimum(np.arange(self.tw) + 1, self.tw - np.arange(self.tw))
        self.tile_elems = self.th * self.tw * self.C

    def tile_id(self, m, i, j):
        return (m * self.ky + i) * self.kx + j

    def tile(self, tid):
        """(m, i, j) of a tile id."""
        m, rest = divmod(int(tid), self.ky * self.kx)
        return (m,) + divmod(rest, self.kx)

    def covering(self, axis, pos):
        """The (contiguous, ascending) indices of the tiles covering position ``pos`` of axis 0 (y) or 1 (x)."""
        o, t = (self.oy, self.th) if axis == 0 else (self.ox, self.tw)
        return [int(i) for i in np.nonzero((o <= pos) & (pos < o + t))[0]]

    def weight(self):
        """[th, tw] integer window weights of a tile."""
        return np.outer(self.w1y, self.w1x)

    def _geom(self):
        return (self.nimg, self.H, self.W, self.C, self.th, self.tw, self.sy, self.sx)


def _images_arg(t, grid, what):
    if t.dtype not in (torch.uint8, torch.float32) or not t.is_cuda:
        raise ValueError("%s must be a uint8 or float32 device tensor" % what)
    if t.numel() != grid.nimg * grid.H * grid.W * grid.C:
        raise ValueError("%s must hold [%d,%d,%d,%d]" % (what, grid.nimg, grid.H, grid.W, grid.C))
    return 1 if t.dtype == torch.uint8 else 0


def extract_tiles(images, grid, first=0, count=None, range=(-1.0, 1.0), out=None):
    """One svae_op_extract_tiles launch on the current stream: ``out`` [count, th, tw, C] float32 (default: a new
    tensor; count defaults to n_tiles) receives tiles first, first + 1, ... (mod n_tiles) of the contiguous uint8
    or float32 device ``images`` [nimg, H, W, C]; uint8 pixels are dequantised into ``range`` as svae_op_make_batch
    does.  Returns ``out``."""
    u8 = _images_arg(images, grid, "images")
    count = grid.n_tiles if count is None else int(count)
    if out is None:
        out = torch.empty([count, grid.th, grid.tw, grid.C], dtype=torch.float32, device=images.device)
    if out.dtype != torch.float32 or out.device != images.device or out.numel() != count * grid.tile_elems:
        raise ValueError("out must be a float32 [count, th, tw, C] tensor on the images' device")
    _lib.check(_lib.lib().svae_op_extract_tiles(
        _lib.ptr(images), u8, *grid._geom(), float(range[0]), float(range[1]), int(first), count, _lib.ptr(out),
        _lib.stream_ptr(torch.cuda.current_stream(images.device))))
    return out


def blend_tiles(tiles, grid, nstack=1, stack_stride=None, source=None, known=None, range=(-1.0, 1.0), out=None,
                out_u8=None, as_uint8=False):
    """One svae_op_blend_tiles launch on the current stream: ``nstack`` sets of all n_tiles tiles (set k at
    ``stack_stride`` floats from set k - 1, default a set's size) of the contiguous float32 device ``tiles`` are
    blended with the window weights into ``out`` (float32) and / or ``out_u8`` (uint8, quantised from ``range``),
    both [nstack, nimg, H, W, C].  With neither given, one is made: uint8 if ``as_uint8``.  Where ``known``
    (uint8 or bool [nimg, H, W]) is non-zero the result is the ``source`` pixel (the layout of the images, uint8 or
    float32).  Returns (out, out_u8)."""
    if tiles.dtype != torch.float32 or not tiles.is_cuda:
        raise ValueError("tiles must be a float32 device tensor")
    nstack = int(nstack)
    stride = grid.n_tiles * grid.tile_elems if stack_stride is None else int(stack_stride)
    if nstack < 1 or tiles.numel() < (nstack - 1) * stride + grid.n_tiles * grid.tile_elems:
        raise ValueError("tiles holds fewer than nstack sets of n_tiles tiles")
    shape = [nstack, grid.nimg, grid.H, grid.W, grid.C]
    if out is None and out_u8 is None:
        if as_uint8:
            out_u8 = torch.empty(shape, dtype=torch.uint8, device=tiles.device)
        else:
            out = torch.empty(shape, dtype=torch.float32, device=tiles.device)
    for t, dt in ((out, torch.float32), (out_u8, torch.uint8)):
        if t is not None and (t.dtype != dt or t.device != tiles.device or t.numel() != int(np.prod(shape))):
            raise ValueError("out / out_u8 must be float32 / uint8 [nstack, nimg, H, W, C] on the tiles' device")
    src_u8 = 0
    if (known is None) != (source is None):
        raise ValueError("known and source come together")
    if known is not None:
        src_u8 = _images_arg(source, grid, "source")
        if known.dtype == torch.bool:
            known = known.to(torch.uint8)
        if known.dtype != torch.uint8 or known.device != tiles.device or known.numel() != grid.nimg * grid.H * grid.W:
            raise ValueError("known must be a uint8 or bool [nimg, H, W] tensor on the tiles' device")
    _lib.check(_lib.lib().svae_op_blend_tiles(
        _lib.ptr(tiles), nstack, stride, *grid._geom(), _lib.ptr(source), src_u8, _lib.ptr(known), float(range[0]),
        float(range[1]), _lib.ptr(out), _lib.ptr(out_u8), _lib.stream_ptr(torch.cuda.current_stream(tiles.device))))
    return out, out_u8


def windows(n_tiles, B):
    """[(first, count, fresh)]: the tile windows of a walk in batches of B, evaluate()'s rule.  first = 0, B, ...;
    with a remainder the last window is first = n_tiles - B, of which only the last ``fresh`` rows are new; with
    n_tiles < B one window (0, B) wraps, its first n_tiles rows are the tiles."""
    if n_tiles < B:
        return [(0, B, n_tiles)]
    w = [(s, B, B) for s in range(0, n_tiles - B + 1, B)]
    if n_tiles % B:
        w.append((n_tiles - B, B, n_tiles % B))
    return w


def _device_images(net, images, what):
    t = images if isinstance(images, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(images))
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    elif t.dtype != torch.uint8:
        if not t.dtype.is_floating_point:
            raise ValueError("%s must be uint8 or floating point, got %s" % (what, t.dtype))
        t = t.to(torch.float32)
    return t.to(net.device).contiguous()


def _replicate(t, H, W):
    """Edge-replicate [N, h, w, ...] up to H x W (bottom and right)."""
    n, h, w = t.shape[:3]
    iy = torch.clamp(torch.arange(H, device=t.device), max=h - 1)
    ix = torch.clamp(torch.arange(W, device=t.device), max=w - 1)
    return t[:, iy][:, :, ix].contiguous()


def restore(net, images, range=(-1.0, 1.0), stride=None, steps=-1, seed=None, known=None, as_uint8=None,
            max_bytes=4 << 30):
    """SequentialVAE.restore (the documentation is there)."""
    cfg = net.cfg
    if getattr(cfg, "external_generator_from", 0):
        raise ValueError("the PixelVAE head is not a trainer network")
    img = _device_images(net, images, "images")
    if img.dim() == 3:
        img = img.unsqueeze(0)
    h, w, C = cfg.height, cfg.width, cfg.channels
    if img.dim() != 4 or img.shape[3] != C:
        raise ValueError("images must be [H,W,%d] or [N,H,W,%d], got %s" % (C, C, tuple(img.shape)))
    N, H0, W0 = (int(v) for v in img.shape[:3])
    if N < 1 or H0 < 1 or W0 < 1:
        raise ValueError("images are empty: %s" % (tuple(img.shape),))
    if as_uint8 is None:
        as_uint8 = img.dtype == torch.uint8
    lo, hi = float(range[0]), float(range[1])
    if not lo < hi:
        raise ValueError("range must be (lo, hi) with lo < hi")
    if stride is None:
        stride = (max(1, h // 2), max(1, w // 2))
    sy, sx = (int(stride),) * 2 if np.isscalar(stride) else (int(stride[0]), int(stride[1]))
    if not (1 <= sy <= h and 1 <= sx <= w):
        raise ValueError("stride must be in 1 .. tile per axis, got (%d, %d) for a %d x %d tile" % (sy, sx, h, w))
    T = cfg.mc_steps
    if isinstance(steps, str):
        if steps != "all":
            raise ValueError("steps must be an int or 'all'")
        which = np.arange(T).tolist()
    else:
        if not -T <= int(steps) < T:
            raise ValueError("steps must be in [-%d, %d)" % (T, T))
        which = [int(steps) % T]
    if known is not None:
        known = _device_images(net, known, "known")
        if known.dtype != torch.uint8:
            raise ValueError("known must be bool or uint8")
        if known.dim() == 2:
            known = known.unsqueeze(0)
        if tuple(known.shape) != (N, H0, W0):
            raise ValueError("known must be [H,W] or [N,H,W] like the images, got %s" % (tuple(known.shape),))
    # an image smaller than the tile is edge-replicated up to it and cropped afterwards
    H, W = max(H0, h), max(W0, w)
    if (H, W) != (H0, W0):
        img = _replicate(img, H, W)
        known = None if known is None else _replicate(known, H, W)
    grid = TileGrid(N, H, W, C, h, w, sy, sx)
    S, B, per = len(which), cfg.batch, h * w * C
    need = 4 * S * grid.n_tiles * per
    if need > max_bytes:
        raise ValueError("restore would keep %d bytes of tiles (%d steps x %d tiles), above max_bytes = %d: "
                         "pass fewer images per call" % (need, S, grid.n_tiles, max_bytes))
    dev = net.device
    with torch.cuda.device(dev):
        if getattr(net, "_restore_inp", None) is None:
            net._restore_inp = torch.empty([B, h, w, C], dtype=torch.float32, device=dev)
            net._restore_rows = torch.empty([B, h, w, C], dtype=torch.float32, device=dev)
        inp, rows = net._restore_inp, net._restore_rows
        kept = getattr(net, "_restore_kept", None)
        if kept is None or kept.numel() < S * grid.n_tiles * per:
            kept = net._restore_kept = torch.empty(S * grid.n_tiles * per, dtype=torch.float32, device=dev)
        kept = kept[:S * grid.n_tiles * per].view(S, grid.n_tiles, h, w, C)
        gen = None if seed is None else torch.Generator(device=dev).manual_seed(int(seed) & 0xFFFFFFFFFFFFFFFF)
        zero_eps = torch.zeros([T, B, cfg.latent_dim], dtype=torch.float32, device=dev) if gen is None else None
        zero_noise = None
        if gen is None and cfg.add_noise_to_chain:
            zero_noise = torch.zeros([T, B, h, w, C], dtype=torch.float32, device=dev)
        stream = _lib.stream_ptr(torch.cuda.current_stream(dev))
        for first, count, fresh in windows(grid.n_tiles, B):
            extract_tiles(img, grid, first, count, (lo, hi), out=inp)
            eps, noise = zero_eps, zero_noise
            if gen is not None:
                eps = torch.randn([T, B, cfg.latent_dim], generator=gen, dtype=torch.float32, device=dev)
                if cfg.add_noise_to_chain:
                    noise = torch.randn([T, B, h, w, C], generator=gen, dtype=torch.float32, device=dev)
            net.forward(inp, inp, eps, 1.0, noise=noise)
            # svae_copy_out copies all B rows: a whole window goes straight into place, the new rows of a partial
            # one (the trailing rows of the last window, the leading rows of a wrapping one) through `rows`
            for k, t in enumerate(which):
                dst = kept[k, first:first + B] if fresh == B else rows
                _lib.check(net.L.svae_copy_out(net.ctx, _lib.BUF_XHAT, t, _lib.ptr(dst), B * per, stream), net.ctx)
                if fresh != B and grid.n_tiles < B:
                    kept[k].copy_(rows[:fresh])
                elif fresh != B:
                    kept[k, grid.n_tiles - fresh:].copy_(rows[B - fresh:])
        out, out_u8 = blend_tiles(kept, grid, nstack=S, source=None if known is None else img, known=known,
                                  range=(lo, hi), as_uint8=as_uint8)
    res = out_u8 if as_uint8 else out
    if (H, W) != (H0, W0):
        res = res[:, :, :H0, :W0].contiguous()
    return res if isinstance(steps, str) else res[0]
