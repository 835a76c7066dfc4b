"""The reference's NoisyTrainer (trainer.py) over a device-resident dataset.

One training iteration is two enqueues: svae_op_make_batch (csrc/batch.hip) gathers the cursor's window from
the dataset in HBM, dequantises it into the clean target and, with denoise_train, corrupts a copy into the
input (pepper x0, salt +1, Gaussian, clip: trainer.py:71-78 on the device instead of three host draws over
the batch in float64); then ``network.train(input, target)``.  Nothing crosses the host in the step but
the returned loss.

Draws are counter-based (Philox, key = seed, counter = offset): training noise and test noise use
different seeds, each offset advances by ceil(B H W C / 4) per corrupted batch, and both are part of
state_dict(), so a resumed run corrupts its next batch exactly as the uninterrupted run would.

With ``degradation`` (a degrade.Degradation) the input is instead the clean target blurred, down-sampled and cut
out per image by svae_op_degrade_batch (csrc/degrade.hip), a second enqueue after a target-only make_batch, under
the same seeds and offsets (its per-image draws come from a Philox stream make_batch leaves unused), followed by
the pixel noise above when denoise_train is on.  A degradation whose ``jpeg`` stage has p > 0 then puts that input
through svae_op_jpeg_batch (csrc/jpeg.hip) in place, a third enqueue under the same seed and offset (Philox stream
5): sensor noise first, then compression.  No new state: state_dict() is what it was.

With a data.PatchDataset the clean training target is instead a batch of fresh random crops of large images
(svae_op_crop_batch, csrc/crops.hip) under the training seed and offset, and the input is derived from it as above;
test batches and every evaluation walk the dataset's fixed sets of crops as they walk any dataset.  No new state
either: train_offset, which is checkpointed, then advances every step.
"""
import json
import logging
import math
import os
import time

import torch

from . import _lib
from . import canvas as cv


class NoisyTrainer:
    # the reference's class constants (trainer.py:16-21)
    pepper_prob = 0.1
    salt_prob = 0.1
    gaussian_noise_scale = 0.1
    max_training_iters = 10000000
    test_num_iters = 5
    log_loss_freq = 20
    save_freq = 2000           # sequential_vae.py:254
    test_seed_xor = 0x7E577E57A5A5A5A5  # test-noise key = seed ^ this
    eval_seed_xor = 0xE7A1E7A15C0DE5ED  # evaluate()'s corruption key = its seed ^ this

    def __init__(self, network, dataset, denoise_train=False, vis_frequency=1000, plot_reconstruction=False,
                 base_dir=None, logger=None, seed=0, summary_freq=0, eval_frequency=0, info_frequency=0,
                 quality_frequency=0, degradation=None, spectrum_frequency=0, ema_decay=None, ema_warmup=True,
                 ema_every=1, quality_k=None):
        if list(dataset.data_dims) != list(network.data_dims):
            raise ValueError("dataset images %s, network %s" % (dataset.data_dims, network.data_dims))
        if tuple(dataset.range) != tuple(float(v) for v in network.cfg.range):
            raise ValueError("dataset range %s, network %s" % (dataset.range, network.cfg.range))
        if getattr(network.cfg, "external_generator_from", 0):
            raise ValueError("the PixelVAE head is not a trainer network")
        self.network = network
        self.dataset = dataset
        # ema_decay: the network keeps Polyak averages of its weights (SequentialVAE.enable_ema), every report takes
        # weights="ema" and the periodic writers report both; None: every launch is exactly what it is without it
        if ema_decay is not None:
            if network.ema is None:
                network.enable_ema(ema_decay, ema_warmup, ema_every)
            elif network.ema_decay != float(ema_decay):
                raise ValueError("the network averages with decay %r, the trainer asks for %r"
                                 % (network.ema_decay, float(ema_decay)))
        self.denoise_train = bool(denoise_train)
        # a degrade.Degradation: every training, test and evaluation input is the clean batch blurred, down-sampled
        # and cut out by svae_op_degrade_batch (csrc/degrade.hip), then given the pixel noise (under denoise_train);
        # None: every launch is exactly what it is without this option
        self.degradation = degradation
        self.vis_frequency = int(vis_frequency)
        self.plot_reconstruction_enabled = bool(plot_reconstruction)
        self.base_dir = base_dir
        self.LOG = logger if logger is not None else logging.getLogger("svae.trainer")
        # every summary_freq-th step appends network.summaries() to <base_dir>/summaries.jsonl (the reference's
        # tb_summary_freq is 10); 0: none, and the step is exactly what it is without this option
        self.summary_freq = int(summary_freq)
        # every eval_frequency-th step appends evaluate() to <base_dir>/evaluation.jsonl; 0: none, and the loop is
        # exactly what it is without this option
        self.eval_frequency = int(eval_frequency)
        # every info_frequency-th step appends latent_information() to <base_dir>/latent_information.jsonl; 0: none,
        # and the loop is exactly what it is without this option
        self.info_frequency = int(info_frequency)
        # every quality_frequency-th step appends sample_quality() to <base_dir>/sample_quality.jsonl; 0: none, and
        # the loop is exactly what it is without this option
        self.quality_frequency = int(quality_frequency)
        # a tuple of k: the periodic sample_quality() carries the k-nearest-neighbour manifold metrics (its
        # manifold_k); None: the report is exactly what it is without this option
        self.quality_k = None if quality_k is None else tuple(int(k) for k in quality_k)
        # every spectrum_frequency-th step appends spectrum() to <base_dir>/spectrum.jsonl; 0: none, and the loop is
        # exactly what it is without this option
        self.spectrum_frequency = int(spectrum_frequency)
        self._eval_stack = self._eval_rows = None  # evaluate()'s kept device buffers
        self._spectrum_buffers = None               # spectrum()'s
        self.batch_size = network.batch_size
        self.data_dims = list(dataset.data_dims)
        self.device = network.device
        if dataset.train.device != self.device or dataset.test.device != self.device:
            raise ValueError("the dataset must live on the network's device (%s)" % self.device)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.iteration = 0
        self.train_offset = 0
        self.test_offset = 0
        shape = [self.batch_size] + self.data_dims
        # one pair, reused: the kernel and the step that reads it are ordered on one stream
        self._target = torch.empty(shape, dtype=torch.float32, device=self.device)
        self._input = torch.empty(shape, dtype=torch.float32, device=self.device)

    # ------------------------------------------------------------------ the batch kernel
    def _groups(self):
        return (self.batch_size * self.dataset.per_image + 3) // 4

    def _make_batch(self, data, start, target, inp, seed, offset, noise=True):
        """One svae_op_make_batch launch on the current stream: rows [start, start + B) of ``data``."""
        lo, hi = self.dataset.range
        p, s, g = (self.pepper_prob, self.salt_prob, self.gaussian_noise_scale) if noise else (0.0, 0.0, 0.0)
        _lib.check(_lib.lib().svae_op_make_batch(
            _lib.ptr(data), 1 if data.dtype == torch.uint8 else 0, None, int(start), self.batch_size,
            self.dataset.per_image, lo, hi, p, s, g, seed, offset & 0xFFFFFFFFFFFFFFFF, _lib.ptr(target),
            _lib.ptr(inp), _lib.stream_ptr(torch.cuda.current_stream(self.device))))

    def _corrupted_batch(self, data, start, seed, offset):
        """The window [start, start + B) of ``data`` as the clean self._target and the network's input; returns
        (input, corrupted).  Without a degradation and without denoise_train the input is the target itself and
        no draw is made (corrupted is False: the caller leaves its offset alone).  With denoise_train alone it is
        svae_op_make_batch's noisy copy under (seed, offset).  With a degradation it is svae_op_degrade_batch of
        the clean target under the same (seed, offset), the pixel noise being the class constants under
        denoise_train and zero otherwise, followed by svae_op_jpeg_batch in place where its jpeg stage has p > 0
        (_degraded).  A corrupting call consumes ceil(B H W C / 4) counters."""
        if self.degradation is None:
            if not self.denoise_train:
                self._make_batch(data, start, self._target, None, 0, 0, noise=False)
                return self._target, False
            self._make_batch(data, start, self._target, self._input, seed, offset)
            return self._input, True
        self._make_batch(data, start, self._target, None, 0, 0, noise=False)
        return self._degraded(seed, offset), True

    def _degraded(self, seed, offset):
        """self._input as the degradation's copy of the clean self._target under (seed, offset):
        svae_op_degrade_batch with the pixel noise of denoise_train, then, where the jpeg stage has p > 0,
        svae_op_jpeg_batch in place on the result (image b under the counter offset + b of Philox stream 5, which no
        other draw of the batch uses).  With jpeg at p = 0 nothing is launched for it."""
        from . import degrade
        lo, hi = self.dataset.range
        noise = (self.pepper_prob, self.salt_prob, self.gaussian_noise_scale) if self.denoise_train else (0.0, 0.0, 0.0)
        degrade.degrade_batch(self._target, self.degradation, lo, hi, noise, seed, offset, out=self._input)
        if self.degradation.jpeg[0] > 0.0:
            degrade.jpeg_batch(self._input, self.degradation, lo, hi, seed, offset)
        return self._input

    def apply_noise(self, batch):
        """The reference's apply_noise on a given fp32 device batch [B,H,W,C], in place (the same kernel
        with input == data); draws from the training stream.  Raises when denoise_train is off, as the
        reference does (trainer.py:66-67)."""
        if not self.denoise_train:
            raise RuntimeError("Called apply_noise, but denoise_train is off")
        if batch.dtype != torch.float32 or batch.device != self.device or not batch.is_contiguous() \
                or list(batch.shape) != [self.batch_size] + self.data_dims:
            raise ValueError("apply_noise takes a contiguous float32 [B,H,W,C] batch on the network's device")
        self._make_batch(batch, 0, None, batch, self.seed, self.train_offset)
        self.train_offset += self._groups()
        return batch

    def _next(self, test=False):
        """The next window as (input, target) device tensors; advances the cursor and, when it corrupts,
        the stream's offset."""
        ds = self.dataset
        if not test and hasattr(ds, "patch_batch"):
            return self._next_patches()
        start, _ = ds.next_test_batch(self.batch_size) if test else ds.next_batch(self.batch_size)
        data = ds.test if test else ds.train
        if test:
            inp, corrupted = self._corrupted_batch(data, start, self.seed ^ self.test_seed_xor, self.test_offset)
            self.test_offset += self._groups() if corrupted else 0
        else:
            inp, corrupted = self._corrupted_batch(data, start, self.seed, self.train_offset)
            self.train_offset += self._groups() if corrupted else 0
        return inp, self._target

    def _next_patches(self):
        """The training batch of a data.PatchDataset: self._target is ``batch_size`` fresh crops of the large
        training images (one svae_op_crop_batch launch under (seed, train_offset + b): Philox stream 4, which neither
        the pixel noise nor the degradation draws from, so the three share the key and the offset), and the input is
        derived from that target as from any other: svae_op_make_batch on the fp32 target under denoise_train alone,
        svae_op_degrade_batch (and svae_op_jpeg_batch: _degraded) under a degradation, the target itself otherwise.
        train_offset advances by one batch in every case (an uncorrupted run would otherwise redraw the same crops); the dataset's train cursor does
        not move."""
        ds = self.dataset
        ds.patch_batch(self.batch_size, self.seed, self.train_offset, self._target)
        inp = self._target
        if self.degradation is not None:
            inp = self._degraded(self.seed, self.train_offset)
        elif self.denoise_train:
            self._make_batch(self._target, 0, None, self._input, self.seed, self.train_offset)
            inp = self._input
        self.train_offset += self._groups()
        return inp, self._target

    # ------------------------------------------------------------------ the reference's loop
    def step(self):
        """One training iteration (trainer.py:100-104); returns network.train's loss."""
        inp, tgt = self._next()
        loss = self.network.train(inp, tgt)
        self.iteration += 1
        if self.summary_freq > 0 and self.iteration % self.summary_freq == 0:
            self.write_summaries()
        if self.eval_frequency > 0 and self.iteration % self.eval_frequency == 0:
            self.write_evaluation()  # after the summaries: they describe the training forward
        if self.info_frequency > 0 and self.iteration % self.info_frequency == 0:
            self.write_latent_information()
        if self.quality_frequency > 0 and self.iteration % self.quality_frequency == 0:
            self.write_sample_quality(**({} if self.quality_k is None else {"manifold_k": self.quality_k}))
        if self.spectrum_frequency > 0 and self.iteration % self.spectrum_frequency == 0:
            self.write_spectrum()
        return loss

    def write_summaries(self):
        """One line {"iteration", "learning_rate", "reg_coeff", <network.summaries()>}: logged at debug level
        and, with a base_dir, appended to <base_dir>/summaries.jsonl (a resumed run goes on in the same file)."""
        net = self.network
        row = {"iteration": self.iteration, "learning_rate": net.learning_rate, "reg_coeff": net._last_reg}
        row.update(net.summaries())
        line = json.dumps(row)
        self.LOG.debug(line)
        if self.base_dir is not None:
            os.makedirs(self.base_dir, exist_ok=True)
            with open(os.path.join(self.base_dir, "summaries.jsonl"), "a") as f:
                f.write(line + "\n")
        return row

    def train(self, num_iters=None):
        """trainer.py:82-109: every vis_frequency iterations test + visualise, every log_loss_freq log,
        every save_freq save a checkpoint (the reference's network saves inside its train, :254)."""
        n = self.max_training_iters if num_iters is None else int(num_iters)
        loss = None
        for _ in range(n):
            it = self.iteration
            t0 = time.time()
            if it % self.vis_frequency == 0:
                err = self.test(it // self.vis_frequency)
                self.LOG.info("Reconstruction error per pixel: %f, @ iteration: %d" % (err, it))
                self.network.visualize(it // self.vis_frequency, self.dataset, self.base_dir)
            loss = self.step()
            if it % self.log_loss_freq == 0:
                self.LOG.info("Iteration %d: Reconstruction loss %f, time per iter %fs" % (it, loss, time.time() - t0))
            if self.base_dir is not None and self.iteration % self.save_freq == 0:
                self.save(self.base_dir)
        return loss

    def test(self, epoch, num_iters=None, weights="train"):
        """Mean over num_iters test batches of sum((recon - clean)^2) / (H W) / B (trainer.py:131), recon
        = training_mles[-1] of forward(noisy, clean).  The engine already reduces mean((mle - target)^2)
        per image (SVAE_BUF_REC_IMG[T-1]), so only B floats are read per batch; under
        predict_generator_noise that buffer holds the NLL and the error is formed from x_hat.  ``weights`` =
        "ema" runs the same batches on the averaged weights (network.averaged())."""
        n = self.test_num_iters if num_iters is None else int(num_iters)
        net = self._net(weights)
        H, W, C = self.data_dims
        T = net.cfg.mc_steps
        err = torch.zeros((), dtype=torch.float64, device=self.device)
        for i in range(n):
            inp, tgt = self._next(test=True)
            net.forward(inp, tgt, None, 1.0)
            if net.cfg.predict_generator_noise:
                err += (net.xhat(-1).double() - tgt.double()).square().sum() / (H * W) / self.batch_size
            else:
                err += net.copy_out(_lib.BUF_REC_IMG, T - 1, self.batch_size).double().mean() * C
            if i == 0 and self.plot_reconstruction_enabled:
                self.plot_reconstruction(epoch, tgt, inp, net.xhat(-1))
        return float(err) / n

    # ------------------------------------------------------------------ held-out evaluation
    def _net(self, weights):
        """The context a report runs on: the training network, or for weights="ema" its averaged() context (its own
        arena: the training context's last forward, like everything else of the run, stays what it was)."""
        if weights not in ("train", "ema"):
            raise ValueError("weights must be 'train' or 'ema', got %r" % (weights,))
        return self.network if weights == "train" else self.network.averaged()

    def _tag(self, res, weights):
        """A report's dict with "weights" ("train" or "ema") added when the network averages; without averaging
        the dict is exactly what it was before the option existed."""
        if self.network.ema is not None:
            res["weights"] = weights
        return res

    def _write_report(self, report, fname, kw):
        """One line {"iteration", <report(**kw)>} logged at info level and, with a base_dir, appended to
        <base_dir>/<fname>; with averaging on and no ``weights`` asked for, one line for the training weights and one
        for the averaged ones.  Returns the first row."""
        which = [kw["weights"]] if "weights" in kw else ["train", "ema"] if self.network.ema is not None else ["train"]
        rows = []
        for w in which:
            row = {"iteration": self.iteration}
            row.update(report(**dict(kw, weights=w)))
            line = json.dumps(row)
            self.LOG.info(line)
            if self.base_dir is not None:
                os.makedirs(self.base_dir, exist_ok=True)
                with open(os.path.join(self.base_dir, fname), "a") as f:
                    f.write(line + "\n")
            rows.append(row)
        return rows[0]

    def _eval_windows(self, split, num_batches, seed, what):
        """The fixed walk that evaluate(), latent_information() and spectrum() share: (data, windows, images, seed)
        for ``split``, windows a list of (start, rows not yet counted) as evaluate() describes them.  Raises for the
        PixelVAE head, a bad split, N < B and an empty walk."""
        net, ds = self.network, self.dataset
        if getattr(net.cfg, "external_generator_from", 0):
            raise ValueError("the PixelVAE head is not a trainer network")
        if split not in ("test", "train"):
            raise ValueError("split must be 'test' or 'train', got %r" % (split,))
        data = ds.test if split == "test" else ds.train
        N, B = int(data.shape[0]), self.batch_size
        if N < B:
            raise ValueError("batch %d exceeds the %d images of the %s split" % (B, N, split))
        seed = self.seed if seed is None else int(seed) & 0xFFFFFFFFFFFFFFFF
        windows = [(s, B) for s in range(0, N - B + 1, B)]  # (start, rows not yet counted)
        if num_batches is not None:
            windows = windows[:max(0, int(num_batches))]
        elif N % B:
            windows.append((N - B, N % B))
        images = sum(f for _, f in windows)
        if images == 0:
            raise ValueError("%s needs at least one window" % what)
        return data, windows, images, seed

    def _eval_forwards(self, data, windows, seed, net=None):
        """The forwards of that walk, one per window, under evaluate()'s draws: the corruption key
        ``seed ^ eval_seed_xor`` from offset 0, eps and then the chain noise from one
        ``torch.Generator(device).manual_seed(seed)``, forward at reg_coeff 1.0.  Yields (input, rows not yet
        counted) with the window's forward as the network's last one and its clean images in self._target.
        ``net``: the context that runs them (default the training network; _net)."""
        net = self.network if net is None else net
        B, T = self.batch_size, net.cfg.mc_steps
        H, W, C = self.data_dims
        gen = torch.Generator(device=self.device).manual_seed(seed)
        offset = 0
        for start, fresh in windows:
            inp, corrupted = self._corrupted_batch(data, start, seed ^ self.eval_seed_xor, offset)
            offset += self._groups() if corrupted else 0
            eps = torch.randn([T, B, net.cfg.latent_dim], generator=gen, dtype=torch.float32, device=self.device)
            noise = None
            if net.cfg.add_noise_to_chain:
                noise = torch.randn([T, B, H, W, C], generator=gen, dtype=torch.float32, device=self.device)
            net.forward(inp, self._target, eps, 1.0, noise=noise)
            yield inp, fresh

    def evaluate(self, split="test", num_batches=None, seed=None, weights="train"):
        """Quality of every chain step on a fixed validation set: the whole ``split`` ("test" or "train"), each
        image once, scored against the clean image in PSNR and SSIM (metrics.image_metrics), with the corrupted
        input as the baseline.

        The split is walked in windows of B from 0; a last partial window is [N - B, N), of which only the rows
        not yet counted enter the means (N < B raises).  ``num_batches`` = k limits the walk to the first k whole
        windows.  Nothing of the training run moves: not the dataset cursors, not train_offset / test_offset,
        not the parameters, the Adam state or the iteration, and not the network's device Philox counter,
        because every draw is injected.  With denoise_train the corruption is svae_op_make_batch under the key
        ``seed ^ eval_seed_xor`` from offset 0 (advancing by one batch per window), with a ``degradation``
        svae_op_degrade_batch under the same key and offsets (_corrupted_batch); eps [T,B,Dz] and then, under
        add_noise_to_chain, the chain noise [T,B,H,W,C] of every window come from one
        ``torch.Generator(device).manual_seed(seed)`` made at the start.  ``seed`` defaults to the trainer's.
        Every evaluation of a split therefore scores the same corrupted images with the same draws.

        Per window: forward(input, target, eps, 1.0, noise), x_hat_t copied into slots 1 .. T of a kept
        [T + 1, B, H, W, C] stack whose slot 0 is the input, one metrics launch, and sums into a device fp64
        table; one device -> host copy at the end.  Returns

            {"split", "images", "seed", "input": {"mse", "psnr", "ssim"},
             "steps": [{"mse", "psnr", "ssim", "recon", "kl"} for every t], "error_per_pixel", "elbo"}

        where every number is a mean over the images: psnr the mean of the per-image values (with L = hi - lo;
        +inf for an image reproduced exactly, as the input is without denoise_train), recon and kl the per-image
        SVAE_BUF_REC_IMG / SVAE_BUF_KL_IMG of step t, error_per_pixel the reference's
        sum (x_hat_{T-1} - x)^2 / (H W) (trainer.py:131), elbo the per-image loss at reg_coeff 1.0.

        Afterwards the network's last forward is the evaluation's last window: summaries() reads the last
        forward, so call it before evaluating (step() does).

        ``weights`` = "ema" scores the Polyak averages instead (network.averaged(), with enable_ema / ema_decay):
        the same windows, seeds and injected draws on a context of its own, so that not even the training
        context's last forward moves.  On a network that averages the result carries "weights" (_tag)."""
        net, ds = self._net(weights), self.dataset
        data, windows, images, seed = self._eval_windows(split, num_batches, seed, "evaluate")
        from . import metrics
        B, T = self.batch_size, net.cfg.mc_steps
        H, W, C = self.data_dims
        lo, hi = ds.range
        L, per = hi - lo, H * W * C
        if self._eval_stack is None:
            self._eval_stack = torch.empty([T + 1, B, H, W, C], dtype=torch.float32, device=self.device)
            self._eval_rows = torch.empty([(T + 1) * B, metrics.COLS], dtype=torch.float64, device=self.device)
        stack, rows = self._eval_stack, self._eval_rows
        # columns: sum of mse, psnr, ssim, recon, kl per slot (slot 0: the input, no recon / kl); elbo beside it
        table = torch.zeros([T + 1, 5], dtype=torch.float64, device=self.device)
        elbo = torch.zeros((), dtype=torch.float64, device=self.device)
        stream = _lib.stream_ptr(torch.cuda.current_stream(self.device))
        for inp, fresh in self._eval_forwards(data, windows, seed, net):
            stack[0].copy_(inp)
            for t in range(T):
                _lib.check(net.L.svae_copy_out(net.ctx, _lib.BUF_XHAT, t, _lib.ptr(stack[1 + t]), B * per, stream),
                           net.ctx)
            m = metrics.image_metrics(stack, self._target, L, out=rows).view(T + 1, B, metrics.COLS)[:, B - fresh:]
            table[:, 0] += (m[:, :, metrics.COL_SSE] / per).sum(1)
            table[:, 1] += metrics.psnr(m[:, :, metrics.COL_SSE], per, L).sum(1)
            table[:, 2] += m[:, :, metrics.COL_SSIM].sum(1)
            for col, which in ((3, _lib.BUF_REC_IMG), (4, _lib.BUF_KL_IMG)):
                per_step = torch.stack([net.copy_out(which, t, B) for t in range(T)])
                table[1:, col] += per_step[:, B - fresh:].double().sum(1)
            elbo += net.elbo_per_image()[B - fresh:].sum()
        host = (torch.cat([table.reshape(-1), elbo.reshape(1)]) / images).cpu().tolist()
        mean = lambda slot, col: host[slot * 5 + col]
        res = {"split": split, "images": images, "seed": seed,
               "input": {"mse": mean(0, 0), "psnr": mean(0, 1), "ssim": mean(0, 2)},
               "steps": [{"mse": mean(1 + t, 0), "psnr": mean(1 + t, 1), "ssim": mean(1 + t, 2),
                          "recon": mean(1 + t, 3), "kl": mean(1 + t, 4)} for t in range(T)]}
        res["error_per_pixel"] = res["steps"][-1]["mse"] * C  # sum / (H W) = mse * C
        res["elbo"] = host[-1]
        return self._tag(res, weights)

    def write_evaluation(self, **kw):
        """One line {"iteration", <evaluate(**kw)>}: logged at info level and, with a base_dir, appended to
        <base_dir>/evaluation.jsonl (a resumed run goes on in the same file).  With averaging on and no ``weights``
        given, a second line reports the averaged weights (_write_report); the first row is returned."""
        return self._write_report(self.evaluate, "evaluation.jsonl", kw)

    # ------------------------------------------------------------------ what the latent code carries
    def latent_information(self, split="test", num_batches=None, seed=None, weights="train"):
        """Per chain step, how much information the latent code carries about the image and how far the aggregate
        posterior is from the prior (latents.information: mutual information, marginal KL, total correlation,
        active units), for the whole code, every ladder level and every single dimension.

        The split is walked exactly as evaluate() walks it: the same windows (a last partial window [N - B, N) of
        which only the rows not yet counted are kept; ``num_batches`` = k the first k whole windows), the same
        corruption key ``seed ^ eval_seed_xor`` from offset 0, the same ``torch.Generator(device).manual_seed(seed)``
        stream with eps drawn first and then the chain noise under add_noise_to_chain, forward at reg_coeff 1.0.
        The report therefore describes the very forwards that evaluate(seed=...) scores, and like it moves nothing
        of the training run: no cursor, no offset, no parameter, no Adam state, not the iteration and not the
        device Philox counter.  It raises as evaluate() does for the PixelVAE head, N < B and a bad split.

        Per window SVAE_BUF_MU, _SIGMA and _Z of every step are copied into kept [T, images, Dz] device tensors;
        after the walk one latents.information per step (the posterior mean is the clipped one,
        clamp(SVAE_BUF_MU, +-latent_mean_clip)) and one device -> host copy.  Returns

            {"split", "images", "seed", "mi_ceiling", "prior_stddev" | None,
             "steps": [{"all": {"mi", "marginal_kl", "kl_sample", "kl", "tc", "active_units"},
                        "levels": [{the same, with that level's tc} for every level],
                        "dims": {"mi": [Dz], "marginal_kl": [Dz], "kl": [Dz]}} for every t],
             "nonfinite"}

        ``mi`` saturates at ``mi_ceiling`` = log(images): see latents.py.  Under use_uniform_prior prior_stddev,
        marginal_kl, kl_sample and kl are None.  Afterwards the network's last forward is the walk's last window.
        ``weights`` as in evaluate(), and so is the "weights" field."""
        net = self._net(weights)
        data, windows, images, seed = self._eval_windows(split, num_batches, seed, "latent_information")
        from . import latents
        B, T, Dz = self.batch_size, net.cfg.mc_steps, net.cfg.latent_dim
        kept = torch.empty([3, T, images, Dz], dtype=torch.float32, device=self.device)  # mu, sigma, z
        done = 0
        for _, fresh in self._eval_forwards(data, windows, seed, net):
            for k, which in enumerate((_lib.BUF_MU, _lib.BUF_SIGMA, _lib.BUF_Z)):
                for t in range(T):
                    kept[k, t, done:done + fresh] = net.latent(which, t)[B - fresh:]
            done += fresh
        clip = float(net.cfg.latent_mean_clip)
        mean = kept[0].clamp(-clip, clip) if math.isfinite(clip) else kept[0]
        prior = None if net.cfg.use_uniform_prior else float(net.cfg.latent_prior_stddev)
        lay = latents.Layout(latents.segments_for(net.cfg))
        host = torch.stack([latents.information(kept[2, t], mean[t], kept[1, t], lay.segments, prior)
                            for t in range(T)]).cpu().tolist()
        steps = [lay.report(row, prior is None) for row in host]
        return self._tag({"split": split, "images": images, "seed": seed, "mi_ceiling": math.log(images),
                          "prior_stddev": prior,
                          "steps": [{k: s[k] for k in ("all", "levels", "dims")} for s in steps],
                          "nonfinite": sum(s["nonfinite"] for s in steps)}, weights)

    def write_latent_information(self, **kw):
        """One line {"iteration", <latent_information(**kw)>}: logged at info level and, with a base_dir, appended
        to <base_dir>/latent_information.jsonl (a resumed run goes on in the same file).  With averaging on and no ``weights``
        given, a second line reports the averaged weights (_write_report); the first row is returned."""
        return self._write_report(self.latent_information, "latent_information.jsonl", kw)

    # ------------------------------------------------------------------ how good the samples are
    def _generated_windows(self, nwin, seed, net=None):
        """sample_quality()'s draws, shared with spectrum(): ``nwin`` calls of network.generate(z, noise) with z
        [T,B,Dz] and then, under add_noise_to_chain, the chain noise [T,B,H,W,C] of every window from one
        ``torch.Generator(device).manual_seed(seed)``.  Yields (window, [x_hat_t for every t]).  ``net`` as in
        _eval_forwards."""
        net = self.network if net is None else net
        B, T = self.batch_size, net.cfg.mc_steps
        H, W, C = self.data_dims
        gen = torch.Generator(device=self.device).manual_seed(seed)
        for w in range(nwin):
            z = torch.randn([T, B, net.cfg.latent_dim], generator=gen, dtype=torch.float32, device=self.device)
            noise = None
            if net.cfg.add_noise_to_chain:
                noise = torch.randn([T, B, H, W, C], generator=gen, dtype=torch.float32, device=self.device)
            yield w, net.generate(z, noise=noise)

    def sample_quality(self, split="test", num_batches=None, seed=None, train_images=None, weights="train",
                       manifold_k=None):
        """Per chain step, how close generated samples x_hat_t are to held-out images and whether they copy
        training images: the kernel MMD^2 two-sample estimate, the leave-one-out 1-nearest-neighbour two-sample
        accuracy and nearest-neighbour distances (quality.two_sample), all on svae_op_pairwise_stats.

        The real set R is the ``split`` ("test" or "train") walked in whole windows of B from 0, clean
        (dequantised, never corrupted); ``num_batches`` = k keeps the first k windows.  A trailing partial window
        is dropped here (unlike evaluate(): every generated window is a whole batch, and the two sets are kept
        alike large); N = images < 2 B raises, since the unbiased estimate needs two points per set and one window
        shares one BatchNorm batch.  The generated sets come from N / B calls of network.generate(z, noise): z
        [T,B,Dz] and then, under add_noise_to_chain, the chain noise [T,B,H,W,C] of every window are drawn from
        one ``torch.Generator(device).manual_seed(seed)`` made at the start (``seed`` defaults to the trainer's),
        z before noise.  z is N(0, 1) also under use_uniform_prior: that is what svae_generate itself draws when
        no z is given, whatever the prior.  Every draw is injected, so nothing of the training run moves: not the
        dataset cursors, not train_offset / test_offset, not the parameters, the Adam state or the iteration, and
        not the network's device Philox counter.  The PixelVAE head and a bad split raise as in evaluate().

        x_hat_t of every window and R are kept as one [T + 1, N, D] device tensor, centred on R's mean row (the
        distances do not change, the inner products' rounding shrinks).  Per step quality.two_sample(X_t, R)
        at the bandwidths sigma0^2 * bandwidth_scales of R, the R-against-R pass computed once.  The memorisation
        check is one nearest-neighbour pass of all (T + 1) N rows against the first ``train_images`` training
        images (default min(train size, N); clean, dequantised window by window): nn_train of a step far below
        nn_train of "real" says the samples sit closer to the training set than held-out images do, which is
        copying.  One device -> host copy at the end.  Returns

            {"split", "images", "seed", "sigma0", "bandwidth_scales", "train_images",
             "real": {"nn_train": {"mean", "median", "min"}},
             "steps": [{"mmd2": [5], "mmd2_at_sigma0", "nn_accuracy": {"samples", "real", "all"},
                        "nn_real": {"mean", "median", "min"}, "nn_train": {...}} for every t],
             "nonfinite"}

        with every distance a per-element RMS, sqrt(d2 / D), and sigma0 in the units of d (not per element).
        generate invalidates the network's last training forward: summaries() must be read before (step() does).
        ``weights`` as in evaluate(), and so is the "weights" field.

        ``manifold_k`` = a tuple of k (None: nothing below is launched or reported) adds the k-nearest-neighbour
        manifold metrics on svae_op_pairwise_knn, which say how the sets differ: every step gains "manifold":
        quality.manifold(X_t, R) = {"k", "precision", "recall", "density", "coverage", "nonfinite"}, R's pass
        against itself done once; "real" gains "manifold_train", R against the first ``train_images`` training
        images, the calibration line (what held-out real images score against the training set; None where
        train_images <= max(k)); and the top level "manifold_k".  N - 1 < max(k) raises.  Their NaN counts enter
        "nonfinite"; the tables join the one device -> host copy."""
        net, ds = self._net(weights), self.dataset
        if getattr(net.cfg, "external_generator_from", 0):
            raise ValueError("the PixelVAE head is not a trainer network")
        if split not in ("test", "train"):
            raise ValueError("split must be 'test' or 'train', got %r" % (split,))
        from . import quality
        data = ds.test if split == "test" else ds.train
        B, T, Dz = self.batch_size, net.cfg.mc_steps, net.cfg.latent_dim
        H, W, C = self.data_dims
        D = H * W * C
        nwin = int(data.shape[0]) // B
        if num_batches is not None:
            nwin = min(nwin, max(0, int(num_batches)))
        N = nwin * B
        if N < 2 * B:
            raise ValueError("sample_quality needs at least two whole windows of %d images, the %s split gives %d"
                             % (B, split, nwin))
        mk = None if manifold_k is None else quality._ks(manifold_k, N, N)
        M = int(ds.train.shape[0])
        M = min(M, N) if train_images is None else int(train_images)
        if M < 1 or M > int(ds.train.shape[0]) or int(ds.train.shape[0]) < B:
            raise ValueError("train_images must be in [1, %d] and the training set hold a batch" % int(ds.train.shape[0]))
        seed = self.seed if seed is None else int(seed) & 0xFFFFFFFFFFFFFFFF
        kept = torch.empty([T + 1, N, D], dtype=torch.float32, device=self.device)  # X_0 .. X_{T-1}, R
        for w, xhats in self._generated_windows(nwin, seed, net):
            self._make_batch(data, w * B, self._target, None, 0, 0, noise=False)
            kept[T, w * B:(w + 1) * B] = self._target.view(B, D)
            for t, xh in enumerate(xhats):
                kept[t, w * B:(w + 1) * B] = xh.reshape(B, D)
        train = torch.empty([M, D], dtype=torch.float32, device=self.device)
        for start in range(0, M, B):
            s = min(start, int(ds.train.shape[0]) - B)
            self._make_batch(ds.train, s, self._target, None, 0, 0, noise=False)
            rows = min(B, M - start)
            train[start:start + rows] = self._target.view(B, D)[start - s:start - s + rows]
        mu = kept[T].double().mean(0).float()
        kept -= mu
        train -= mu
        R = kept[T]
        bw = quality.bandwidths(R)
        bwl = bw.tolist()  # (the one early device -> host copy: the op takes the bandwidths on the host)
        yy = quality.self_sums(R, bwl)
        tables = [quality.two_sample_device(kept[t], R, bwl, yy=yy) for t in range(T)]
        _, nd, _ = quality.pairwise_stats(kept.view((T + 1) * N, D), [train], [], ksum=False)
        rms = (nd.view(T + 1, N) / D).sqrt()
        nnt = torch.stack([rms.mean(1), quality.median(rms), rms.min(1).values, torch.isnan(rms).sum(1).double()], 1)
        flat = [torch.stack(tables).reshape(-1), nnt.reshape(-1)]
        if mk is not None:
            ry = quality.self_radii(R, mk)
            flat += [quality.manifold_device(kept[t], R, mk, yy=ry) for t in range(T)]
            if M > max(mk):
                flat.append(quality.manifold_device(R, train, mk))
        host = torch.cat(flat).cpu().tolist()
        nb = len(bwl)
        width = nb + 7
        nn_train = lambda i: dict(zip(("mean", "median", "min"), host[T * width + 4 * i:T * width + 4 * i + 3]))
        steps, bad = [], 0
        for t in range(T):
            r = quality.unpack(host[t * width:(t + 1) * width], nb)
            bad += r["nonfinite"] + int(host[T * width + 4 * t + 3])
            a = r["nn_accuracy"]
            steps.append({"mmd2": r["mmd2"], "mmd2_at_sigma0": r["mmd2_at_sigma0"],
                          "nn_accuracy": {"samples": a["x"], "real": a["y"], "all": a["all"]},
                          "nn_real": r["nn_other"], "nn_train": nn_train(t)})
        bad += int(host[T * width + 4 * T + 3])
        rep = {"split": split, "images": N, "seed": seed, "sigma0": bwl[nb // 2] ** 0.5,
               "bandwidth_scales": list(quality.SCALES), "train_images": M,
               "real": {"nn_train": nn_train(T)}, "steps": steps, "nonfinite": bad}
        if mk is not None:
            mw, at = 4 * len(mk) + 1, T * width + 4 * (T + 1)
            for t in range(T):
                steps[t]["manifold"] = quality.unpack_manifold(host[at + t * mw:at + (t + 1) * mw], mk)
                rep["nonfinite"] += steps[t]["manifold"]["nonfinite"]
            rep["real"]["manifold_train"] = None
            if M > max(mk):
                rep["real"]["manifold_train"] = quality.unpack_manifold(host[at + T * mw:at + (T + 1) * mw], mk)
                rep["nonfinite"] += rep["real"]["manifold_train"]["nonfinite"]
            rep["manifold_k"] = list(mk)
        return self._tag(rep, weights)

    def write_sample_quality(self, **kw):
        """One line {"iteration", <sample_quality(**kw)>}: logged at info level and, with a base_dir, appended to
        <base_dir>/sample_quality.jsonl (a resumed run goes on in the same file).  With averaging on and no ``weights``
        given, a second line reports the averaged weights (_write_report); the first row is returned."""
        return self._write_report(self.sample_quality, "sample_quality.jsonl", kw)

    # ------------------------------------------------------------------ at which frequencies the outputs fail
    def spectrum(self, split="test", num_batches=None, seed=None, samples=True, window="hann", weights="train"):
        """Per chain step, the radially averaged power spectrum of the outputs x_hat_t and of their error against
        the clean images, beside the clean images' own spectrum (spectra.power_spectrum on
        svae_op_power_spectrum): at which spatial frequencies step t still fails, and whether its outputs and the
        generated samples are as sharp as real images.  PSNR and SSIM both reward a smooth output; this report
        does not.

        The split is walked exactly as evaluate() walks it: the same windows (a last partial window [N - B, N) of
        which only the rows not yet counted are kept; ``num_batches`` = k the first k whole windows), the same
        corruption key ``seed ^ eval_seed_xor`` from offset 0, the same ``torch.Generator(device).manual_seed(seed)``
        stream with eps drawn first and then the chain noise under add_noise_to_chain, forward at reg_coeff 1.0.
        The report therefore describes the very forwards that evaluate(seed=...) scores, and like it moves nothing
        of the training run: no cursor, no offset, no parameter, no Adam state, not the iteration and not the
        device Philox counter.  It raises as evaluate() does for the PixelVAE head, N < B and a bad split.

        Per window the kept [T + 1, B, H, W, C] stack (slot 0 the input, slots 1 .. T the x_hat_t) is scored
        against the clean images in one launch and the clean images themselves in a second one (y = None); with
        ``samples`` the whole windows are then generated again as sample_quality() draws them (z [T,B,Dz], then
        the chain noise, from a second generator under the same seed) and scored alone.  ``window`` is "hann"
        (periodic, the default: an image is not periodic, and without a window its edges leak into every
        frequency) or "none".  Sums go into a device fp64 table; one device -> host copy at the end.  Returns

            {"split", "images", "seed", "window", "bins", "counts", "target": {"power_db"},
             "input": {"power_db", "band_snr_db", "log_spectral_distance", "hf_ratio", "cutoff"},
             "steps": [{the same} for every t], "sample_images",
             "samples": [{"power_db", "log_spectral_distance", "hf_ratio"} for every t], "nonfinite"}

        with the channels summed and means over the images.  ``bins`` are the annuli's radii in cycles per pixel
        (b / min(H, W), up to 1/2), ``counts`` their numbers of spectrum entries.  power_db[b] is 10 log10 of the
        mean power per entry of annulus b; band_snr_db[b] = 10 log10(target power / error power) there;
        log_spectral_distance the RMS over b >= 1 of the dB difference to the target's profile; hf_ratio the power
        in the bins above n_bins / 2 over the target's (1: as sharp as the data, below 1: blurred); cutoff the first
        b >= 1 whose band SNR is below 0 dB, over n_bins (1.0: none: every annulus is closer to the clean image than
        a blank one would be).  ``nonfinite`` is the number of non-finite elements among the inputs, outputs, clean
        images and samples that were scored, each counted once (0 in a healthy run).
        Afterwards the network's last forward is the walk's last window, or invalid after the samples:
        summaries() must be read before (step() does).  ``weights`` as in evaluate(), and so is the "weights" field."""
        net = self._net(weights)
        data, windows, images, seed = self._eval_windows(split, num_batches, seed, "spectrum")
        from . import spectra
        B, T = self.batch_size, net.cfg.mc_steps
        H, W, C = self.data_dims
        per = H * W * C
        nb, counts = spectra.device_tables(H, W, window, self.device)[5:7]
        f64 = dict(dtype=torch.float64, device=self.device)
        if self._spectrum_buffers is None:  # kept like evaluate()'s: a report every k-th step allocates once
            self._spectrum_buffers = (torch.empty([T + 1, B, H, W, C], dtype=torch.float32, device=self.device),
                                      torch.empty([(T + 1) * B, C, 2, nb], **f64), torch.zeros([B, C, 2, nb], **f64),
                                      torch.zeros([T + 2, B, C], dtype=torch.int64, device=self.device))
        stack, rows, trow, bad = self._spectrum_buffers
        table = torch.zeros([T + 1, 2, nb], **f64)   # per slot: the power and the error power, summed
        ttable = torch.zeros([nb], **f64)            # the clean images' power
        stable = torch.zeros([T, nb], **f64)         # the generated samples' power
        nonfinite = torch.zeros((), dtype=torch.int64, device=self.device)
        stream = _lib.stream_ptr(torch.cuda.current_stream(self.device))
        for inp, fresh in self._eval_forwards(data, windows, seed, net):
            stack[0].copy_(inp)
            for t in range(T):
                _lib.check(net.L.svae_copy_out(net.ctx, _lib.BUF_XHAT, t, _lib.ptr(stack[1 + t]), B * per, stream),
                           net.ctx)
            r = spectra.power_spectrum(stack, self._target, window, out=rows, nonfinite=bad[:T + 1])
            table += r.view(T + 1, B, C, 2, nb)[:, B - fresh:].sum((1, 2))
            tr = spectra.power_spectrum(self._target, None, window, out=trow, nonfinite=bad[T + 1])
            ttable += tr[B - fresh:, :, 0].sum((0, 1))
            # a stack row's count includes its partner's: the clean images count once, from their own launch
            nonfinite += bad[:T + 1, B - fresh:].sum() - T * bad[T + 1, B - fresh:].sum()
        sample_images = 0
        if samples:
            nwin = sum(1 for _, fresh in windows if fresh == B)
            for _, xhats in self._generated_windows(nwin, seed, net):
                for t, xh in enumerate(xhats):
                    stack[1 + t].copy_(xh)
                r = spectra.power_spectrum(stack[1:], None, window, out=rows, nonfinite=bad[:T])
                stable += r.view(T, B, C, 2, nb)[:, :, :, 0].sum((1, 2))
                nonfinite += bad[:T].sum()
            sample_images = nwin * B
        host = torch.cat([table.reshape(-1) / images, ttable / images, stable.reshape(-1) / max(sample_images, 1),
                          nonfinite.double().reshape(1)]).cpu().tolist()
        slot = lambda s, plane: host[(2 * s + plane) * nb:(2 * s + plane + 1) * nb]
        target = host[2 * (T + 1) * nb:(2 * T + 3) * nb]
        sample = lambda t: host[(2 * T + 3 + t) * nb:(2 * T + 4 + t) * nb]
        entry = lambda s: spectra.profile_report(slot(s, 0), target, counts, err=slot(s, 1))
        res = {"split": split, "images": images, "seed": seed, "window": window,
               "bins": [b / min(H, W) for b in range(nb)], "counts": [float(v) for v in counts],
               "target": {"power_db": spectra.profile_report(target, target, counts)["power_db"]},
               "input": entry(0), "steps": [entry(1 + t) for t in range(T)], "sample_images": sample_images,
               "samples": [spectra.profile_report(sample(t), target, counts) for t in range(T)] if sample_images
               else [], "nonfinite": int(host[-1])}
        return self._tag(res, weights)

    def write_spectrum(self, **kw):
        """One line {"iteration", <spectrum(**kw)>}: logged at info level and, with a base_dir, appended to
        <base_dir>/spectrum.jsonl (a resumed run goes on in the same file).  With averaging on and no ``weights``
        given, a second line reports the averaged weights (_write_report); the first row is returned."""
        return self._write_report(self.spectrum, "spectrum.jsonl", kw)

    def plot_reconstruction(self, train_epoch, original_images, noisy_images, reconstructed_images, num_plot=3):
        """original | noisy | reconstruction of the first num_plot images (canvas.reconstruction_canvas);
        written to <base_dir>/reconstruction/{current, epoch<N>} and returned."""
        disp = lambda a: self.dataset.display(a).cpu().numpy() if isinstance(a, torch.Tensor) else self.dataset.display(a)
        c = cv.reconstruction_canvas(disp(original_images), disp(noisy_images), disp(reconstructed_images), num_plot)
        if self.base_dir is not None:
            folder = self.base_dir + "/reconstruction"
            cv.save_canvas(c, folder, "current")
            cv.save_canvas(c, folder, "epoch%d" % train_epoch)
        return c

    # ------------------------------------------------------------------ resume
    def state_dict(self):
        return {"iteration": self.iteration, "train_offset": self.train_offset, "test_offset": self.test_offset,
                "seed": self.seed, "denoise_train": self.denoise_train, **self.dataset.state_dict()}

    def load_state_dict(self, s):
        self.iteration = int(s["iteration"])
        self.train_offset, self.test_offset = int(s["train_offset"]), int(s["test_offset"])
        self.seed = int(s.get("seed", self.seed))
        self.dataset.load_state_dict(s)

    def save(self, base_dir):
        """The network's checkpoint and, next to it, the trainer's state as JSON."""
        os.makedirs(base_dir, exist_ok=True)
        self.network.save_checkpoint(os.path.join(base_dir, "model.safetensors"))
        with open(os.path.join(base_dir, "trainer.json"), "w") as f:
            json.dump(self.state_dict(), f)

    def load(self, base_dir):
        self.network.load_checkpoint(os.path.join(base_dir, "model.safetensors"))
        with open(os.path.join(base_dir, "trainer.json")) as f:
            self.load_state_dict(json.load(f))
