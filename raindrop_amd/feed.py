"""Batch feed from a device-resident dataset.

The reference slices every training batch on the host and copies it to the GPU
(`code/Raindrop.py:310-315`: `Ptrain_tensor[:, idx, :].cuda()` ... four fancy-index + H2D transfers per
step, 4.4 MB at P19/B=256) and pushes the WHOLE validation split through one forward
(`code/utils_rd.py:310-320`).  With the hot path at ~1 ms per step that host work dominates, so the
dataset is kept in HBM and a batch is one `rd_batch_gather` launch (bit-exact copies + `lengths`):

    ds = DeviceDataset(Ptrain_tensor, Ptrain_time_tensor, Ptrain_static_tensor, ytrain_tensor)
    for idx in epoch_index_plan(ytrain, batch_size=128, strategy=2):        # Raindrop.py:262-307
        P, Pstatic, Ptime, y, lengths = ds.batch(idx)                        # Raindrop.py:310-317
        outputs, _, _ = model.forward(P, Pstatic, Ptime, lengths)
    logits = evaluate_chunked(model, val_ds)                                 # utils_rd.py:310-320

The index plan is the reference's own host logic (same numpy calls in the same order, so the same
`np.random.seed` gives the same batches); only the data movement changed.
"""
import ctypes

import numpy as np
import torch

from . import _lib


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


class Augment:
    """Train-time input augmentation inside the batch gather (rd_feed_gather_aug / rd_batch_gather_aug; DESIGN §3e'): `p_time` drops
    time steps (the kept ones are compacted, `lengths` follows), `p_sensor` whole sensors of a sample, `p_obs` single observations
    -- value and observed-indicator both become 0 --, `value_noise` = sigma jitters the values still observed by a zero-mean
    Irwin-Hall(4) variate of deviation sigma (bounded at 2 sqrt(3) sigma).  Rates in [0, 1), sigma >= 0; a rate of 0 turns its
    transform off.  Every decision is a pure function of (seed, epoch, cursor) and the element's place in the SOURCE sample, so a
    replay reproduces it and tests/feed_aug_ref.py restates it on the host.  Training input only: no evaluation path augments.
    Under data parallelism each rank owns its feed: give each rank its own `seed`, or all ranks draw the same masks."""
    RATES = ("p_time", "p_sensor", "p_obs")

    def __init__(self, p_time=0.0, p_sensor=0.0, p_obs=0.0, value_noise=0.0, seed=0):
        self.p_time, self.p_sensor, self.p_obs, self.value_noise, self.seed = p_time, p_sensor, p_obs, value_noise, seed
        self.check()

    def check(self):
        for name in self.RATES:
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)) or not 0.0 <= float(v) < 1.0:
                raise ValueError("Augment: %s must be a number in [0, 1), got %r" % (name, v))
            if float(v) > 0.0 and float(np.float32(v)) >= 1.0:
                raise ValueError("Augment: %s = %r rounds to 1 in float32" % (name, v))
            setattr(self, name, float(v))
        s = self.value_noise
        if isinstance(s, bool) or not isinstance(s, (int, float, np.floating, np.integer)) or not 0.0 <= float(s) < float("inf"):
            raise ValueError("Augment: value_noise (sigma) must be a finite number >= 0, got %r" % (s,))
        self.value_noise = float(s)
        if isinstance(self.seed, bool) or not isinstance(self.seed, (int, np.integer)):
            raise ValueError("Augment: seed must be an integer, got %r" % (self.seed,))
        self.seed = int(self.seed) & 0xFFFFFFFFFFFFFFFF

    @property
    def noise_c(self):
        """float32(sqrt(3) * sigma): formed in double, rounded once -- the factor the kernel multiplies (s - 2) by"""
        return np.float32(np.sqrt(np.float64(3.0)) * np.float64(self.value_noise))

    def cell(self, epoch=0):
        """the 32-byte device cell {u64 seed, u64 epoch, f32 p_time, f32 p_sensor, f32 p_obs, f32 noise_c} as int64[4] (host)"""
        host = np.zeros(4, dtype=np.int64)
        host.view(np.uint64)[:2] = (self.seed, int(epoch) & 0xFFFFFFFFFFFFFFFF)
        host.view(np.float32)[4:] = (self.p_time, self.p_sensor, self.p_obs, self.noise_c)
        return host

    def state(self):
        return dict(p_time=self.p_time, p_sensor=self.p_sensor, p_obs=self.p_obs, value_noise=self.value_noise, seed=self.seed)

    def __repr__(self):
        return "Augment(%s)" % ", ".join("%s=%r" % kv for kv in self.state().items())


class DeviceDataset:
    """P [T,N,2F] f32, Ptime [T,N] f32, Pstatic [N,d_static] f32 or None, y [N] int64 or None -- moved to
    `device` once.  `batch(idx)` returns freshly allocated (P, Pstatic, Ptime, y, lengths) for the index
    vector `idx` (numpy / list / tensor), or fills the buffers of a previous call when `out=` is given."""

    def __init__(self, P, Ptime, Pstatic=None, y=None, device="cuda"):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise _lib.RaindropHipError("DeviceDataset needs a ROCm device (there is no CPU fallback)")
        self.dev = dev
        self.P = torch.as_tensor(P, dtype=torch.float32).to(dev).contiguous()
        self.Ptime = torch.as_tensor(Ptime, dtype=torch.float32).to(dev).contiguous()
        self.Pstatic = None if Pstatic is None else torch.as_tensor(Pstatic, dtype=torch.float32).to(dev).contiguous()
        self.y = None if y is None else torch.as_tensor(y).reshape(-1).to(torch.int64).to(dev).contiguous()
        self.T, self.N, self.W = self.P.shape
        if tuple(self.Ptime.shape) != (self.T, self.N):
            raise ValueError("Ptime must be [T,N] = [%d,%d], got %s" % (self.T, self.N, tuple(self.Ptime.shape)))
        self.ds = 0 if self.Pstatic is None else int(self.Pstatic.shape[1])
        if self.Pstatic is not None and self.Pstatic.shape[0] != self.N:
            raise ValueError("Pstatic must have N=%d rows" % self.N)
        if self.y is not None and self.y.numel() != self.N:
            raise ValueError("y must have N=%d entries" % self.N)
        self._bad = torch.zeros(1, dtype=torch.int32, device=dev)

    def __len__(self):
        return self.N

    def alloc(self, B):
        f32 = dict(dtype=torch.float32, device=self.dev)
        return {"P": torch.empty((self.T, B, self.W), **f32), "Ptime": torch.empty((self.T, B), **f32),
                "Pstatic": None if self.Pstatic is None else torch.empty((B, self.ds), **f32),
                "y": None if self.y is None else torch.empty((B,), dtype=torch.int64, device=self.dev),
                "lengths": torch.empty((B,), dtype=torch.int64, device=self.dev)}

    def batch(self, idx, out=None, check=True, augment=None, draw=0):
        """augment: an `Augment` -- the batch is gathered by rd_batch_gather_aug under the key `augment.seed + draw` (the eager,
        explicit-index form of what a feed with `augment=` does at draw = epoch * capacity + cursor).  None: the plain gather."""
        if augment is not None and not isinstance(augment, Augment):
            raise ValueError("augment must be None or a feed.Augment, got %r" % (augment,))
        idx_t = torch.as_tensor(np.asarray(idx) if not torch.is_tensor(idx) else idx).reshape(-1).to(torch.int64)
        if check and idx_t.device.type == "cpu" and idx_t.numel():      # host indices: validate for free
            lo, hi = int(idx_t.min()), int(idx_t.max())
            if lo < 0 or hi >= self.N:
                raise IndexError("batch index out of range [0,%d): min %d max %d" % (self.N, lo, hi))
        idx_t = idx_t.to(self.dev)
        B = idx_t.numel()
        o = out if out is not None else self.alloc(B)
        if o["P"].shape[1] != B:
            raise ValueError("out buffers hold %d samples, idx has %d" % (o["P"].shape[1], B))
        if augment is not None:
            cell = torch.from_numpy(augment.cell()).to(self.dev)
            _lib.call("rd_batch_gather_aug", self.T, B, self.W, self.ds, self.N, _p(self.P), _p(self.Ptime), _p(self.Pstatic),
                      _p(self.y), _p(idx_t), _p(o["P"]), _p(o["Ptime"]), _p(o["Pstatic"]), _p(o["y"]), _p(o["lengths"]),
                      _p(self._bad), _p(cell), ctypes.c_uint64(int(draw) & 0xFFFFFFFFFFFFFFFF),
                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
            return o["P"], o["Pstatic"], o["Ptime"], o["y"], o["lengths"]
        _lib.call("rd_batch_gather", self.T, B, self.W, self.ds, self.N, _p(self.P), _p(self.Ptime), _p(self.Pstatic),
                  _p(self.y), _p(idx_t), _p(o["P"]), _p(o["Ptime"]), _p(o["Pstatic"]), _p(o["y"]), _p(o["lengths"]),
                  _p(self._bad), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        return o["P"], o["Pstatic"], o["Ptime"], o["y"], o["lengths"]

    def bad_indices(self):
        """Number of out-of-range indices clamped by batch() since the last call of this method (device-side
        index vectors are not checked on the host); reading it synchronises."""
        n = int(self._bad.item())
        self._bad.zero_()
        return n


class EpochFeed:
    """The batches of one epoch as a device-resident plan that a captured step reads by itself (`TrainStep(..., feed=)`): the
    step's FIRST launch (rd_feed_gather) copies batch `cursor` of the plan out of `ds` into the step's batch buffers, its LAST
    (rd_feed_record) stores the loss and the number of correctly classified samples of that batch and moves the cursor on.  Plan
    and cursor are read on the device when the kernels run, so an epoch is `n_batches` replays of one graph, one small upload
    (`load_epoch`) and one small read-back (`history`); a new epoch, with another number of batches, needs no new capture.

        fd = EpochFeed(ds, batch_size=128, capacity=planner.n_batches)
        step = TrainStep(model, flat, batch, feed=fd); step.capture_full(opt)     # batch: the step's own buffers, any valid contents
        fd.load_epoch(planner.next_epoch())
        while fd.remaining(): step.run_full()
        loss, correct = fd.history()

    Owns one int64 buffer {cursor, n_batches | plan [capacity, batch_size]}, the history [2, capacity] (fp32 losses, int32 counts) and the
    bad-index counter.  `ds` must carry labels.  Under data parallelism every rank has its own feed and loads its own plan rows.

    augment: an `Augment` -- the gather is rd_feed_gather_aug, which augments the batch while it forms it under the key
    `seed + epoch * capacity + cursor`.  The feed then owns the 32-byte cell {seed, epoch, rates}: `load_epoch` writes the next epoch
    number into it (0 for the first), `set_augment` / `set_epoch` rewrite it, all as small copies in stream order -- the captured
    step reads the cell when it runs, so none of them needs a new capture.  A micro-batch of an accumulating step is one cursor
    position and so one draw.  Each rank of a data-parallel run passes its own `seed`.  None (the default): nothing is allocated
    and the launches are the plain feed's."""

    def __init__(self, ds, batch_size, capacity, augment=None):
        if torch.device(ds.dev).type != "cuda":
            raise _lib.RaindropHipError("EpochFeed needs a ROCm device (there is no CPU fallback)")
        if ds.y is None:
            raise _lib.RaindropHipError("EpochFeed needs the dataset's labels (DeviceDataset(..., y=...))")
        self.ds, self.dev, self.B, self.capacity = ds, ds.dev, int(batch_size), int(capacity)
        if self.B <= 0 or self.capacity <= 0:
            raise ValueError("batch_size and capacity must be positive, got %r and %r" % (batch_size, capacity))
        self._state = torch.zeros(2 + self.capacity * self.B, dtype=torch.int64, device=self.dev)
        self.cell, self.plan = self._state[:2], self._state[2:].view(self.capacity, self.B)
        self._hist = torch.zeros((2, self.capacity), dtype=torch.int32, device=self.dev)
        self.loss_hist, self.correct_hist = self._hist[0].view(torch.float32), self._hist[1]
        self._bad = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self._n = self._left = 0
        if augment is not None and not isinstance(augment, Augment):
            raise ValueError("augment must be None or a feed.Augment, got %r" % (augment,))
        self.augment, self._aug, self._epoch = None, None, 0
        if augment is not None:
            if ds.W % 2:
                raise ValueError("augmentation needs W = 2F columns (values | indicators), the dataset has W = %d" % ds.W)
            self.augment = Augment(**augment.state())                  # the feed's own copy: set_augment changes it
            self._aug = torch.from_numpy(self.augment.cell(0)).to(self.dev)
            self._epoch = -1                                           # the first load_epoch is epoch 0

    def _write_aug(self):
        self._aug.copy_(torch.from_numpy(self.augment.cell(max(self._epoch, 0))))

    def set_augment(self, **rates):
        """new rates / sigma / seed (Augment's keywords; the others stay) from the next enqueued step on: one 32-byte copy in
        stream order, no new capture"""
        if self.augment is None:
            raise _lib.RaindropHipError("set_augment: this feed was built without augment=")
        unknown = set(rates) - set(self.augment.state())
        if unknown:
            raise ValueError("set_augment: unknown keywords %s" % sorted(unknown))
        self.augment = Augment(**dict(self.augment.state(), **rates))
        self._write_aug()

    def set_epoch(self, e):
        """the epoch number of the batch key from the next enqueued step on (the next `load_epoch` continues with e + 1)"""
        if self.augment is None:
            raise _lib.RaindropHipError("set_epoch: this feed was built without augment=")
        if isinstance(e, bool) or not isinstance(e, (int, np.integer)) or e < 0:
            raise ValueError("set_epoch: a non-negative integer, got %r" % (e,))
        self._epoch = int(e)
        self._write_aug()

    def augment_state(self):
        """rates, sigma, seed and the epoch number the device cell holds (host mirror, no synchronisation); None without augment="""
        return None if self.augment is None else dict(self.augment.state(), epoch=max(self._epoch, 0))

    def load_epoch(self, batches):
        """`batches`: index vectors of `batch_size` samples each (EpochPlanner.next_epoch()), at most `capacity` of them, checked
        against [0, N) on the host (IndexError).  One host-to-device copy of {0, n | rows}, and the history slots 0 .. n-1 zeroed,
        in the order of the current stream: whatever was enqueued before still sees the previous epoch."""
        rows = [np.asarray(b.cpu() if torch.is_tensor(b) else b).reshape(-1) for b in batches]
        n = len(rows)
        if n > self.capacity:
            raise ValueError("%d batches do not fit a plan of capacity %d" % (n, self.capacity))
        if any(r.size != self.B for r in rows):
            raise ValueError("every batch must hold batch_size = %d indices, got %s" % (self.B, sorted({int(r.size) for r in rows})))
        host = np.zeros(2 + n * self.B, dtype=np.int64)
        host[1] = n
        if n:
            idx = host[2:].reshape(n, self.B)
            idx[:] = np.stack(rows)
            lo, hi = int(idx.min()), int(idx.max())
            if lo < 0 or hi >= self.ds.N:
                raise IndexError("batch index out of range [0,%d): min %d max %d" % (self.ds.N, lo, hi))
        self._state[:host.size].copy_(torch.from_numpy(host))
        if n:
            self._hist[:, :n].zero_()
        self._n = self._left = n
        if self.augment is not None:                                   # a refused plan (above) leaves the epoch where it was
            self._epoch += 1
            self._write_aug()

    def remaining(self):
        """batches of the loaded epoch no step has taken yet: the host's mirror of the device cursor, no synchronisation"""
        return self._left

    def _take(self, who):
        """a step is about to be enqueued: refuse behind the last batch, else count it"""
        if self._left == 0:
            raise _lib.RaindropHipError("%s: the epoch plan is used up (%d of %d batches taken): EpochFeed.load_epoch first"
                                        % (who, self._n, self._n))
        self._left -= 1

    def history(self):
        """(loss [n_done] float32, correct [n_done] int32) of the batches taken so far in this epoch, as numpy arrays: ONE
        device-to-host copy (it waits for the stream)."""
        h = self._hist[:, :self._n - self._left].cpu().numpy()
        return h[0].view(np.float32).copy(), h[1].copy()

    def bad_indices(self):
        """Out-of-range sample indices and cursors the gathers clamped since the last call of this method (`load_epoch` checks the
        indices on the host: anything here came from a plan or cell written some other way); reading it synchronises."""
        n = int(self._bad.item())
        self._bad.zero_()
        return n

    # ---- what a step enqueues (raindrop_amd.step.TrainStep) -------------------------------------------------------------------
    def check_step(self, model, batch):
        """the feed writes into `batch`: same device, same shapes, labels there"""
        ds, src = self.ds, batch["src"]
        if batch.get("y") is None:
            raise ValueError("a fed step needs batch['y']: the feed gathers the labels")
        want = (ds.T, self.B, ds.W)
        if tuple(src.shape) != want or src.device != self.cell.device:
            raise ValueError("the feed gathers src %s on %s, the step's batch holds %s on %s" % (want, self.cell.device, tuple(src.shape), src.device))
        st = batch.get("static")
        if st is not None and (ds.Pstatic is None or tuple(st.shape) != (self.B, ds.ds)):
            raise ValueError("the step's batch has static features %s, the feed's dataset %s" % (
                tuple(st.shape), None if ds.Pstatic is None else (self.B, ds.ds)))

    def enqueue_gather(self, batch, call=_lib.call):
        ds, st = self.ds, batch.get("static")
        if self._aug is not None:
            call("rd_feed_gather_aug", ds.T, self.B, ds.W, ds.ds if st is not None else 0, ds.N, self.capacity, _p(ds.P), _p(ds.Ptime),
                 _p(ds.Pstatic) if st is not None else None, _p(ds.y), _p(self.plan), _p(self.cell), _p(batch["src"]), _p(batch["times"]),
                 _p(st), _p(batch["y"]), _p(batch["lengths"]), _p(self._bad), _p(self._aug),
                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
            return
        call("rd_feed_gather", ds.T, self.B, ds.W, ds.ds if st is not None else 0, ds.N, self.capacity, _p(ds.P), _p(ds.Ptime),
             _p(ds.Pstatic) if st is not None else None, _p(ds.y), _p(self.plan), _p(self.cell), _p(batch["src"]), _p(batch["times"]),
             _p(st), _p(batch["y"]), _p(batch["lengths"]), _p(self._bad), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    def enqueue_record(self, loss, logits, y, call=_lib.call):
        call("rd_feed_record", int(logits.shape[0]), int(logits.shape[1]), self.capacity, _p(self.cell), _p(loss), _p(logits), _p(y),
             _p(self.loss_hist), _p(self.correct_hist), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    def snapshot(self):
        """cursor, history and counter as they are now (device clones, stream-ordered): a capture's warm-up passes run the step
        for real, `restore` puts back what they moved.  (The augmentation cell is not part of it: no step writes it, and a batch's
        masks depend on (seed, epoch, cursor) alone, so a restored cursor draws what it would have drawn.)"""
        return self.cell.clone(), self._hist.clone(), self._bad.clone()

    def restore(self, snap):
        for dst, src in zip((self.cell, self._hist, self._bad), snap):
            dst.copy_(src)


class EpochPlanner:
    """The reference's batch plan over a whole RUN (`code/Raindrop.py:261-307`): `idx_0` and the 3x-expanded `idx_1` are
    created once per run and shuffled IN PLACE at the start of every epoch, so epoch k's permutation is applied on top of
    epoch k-1's.  `next_epoch()` returns the batches of the next epoch; with the same `np.random.seed` the sequence of
    batches over ALL epochs equals the script's (`epoch_index_plan` rebuilds the arrays and therefore only reproduces the
    FIRST epoch of a run)."""

    def __init__(self, ytrain, batch_size=128, strategy=2, n_total=None):
        y = np.asarray(ytrain).reshape(-1)
        self.idx_0 = np.where(y == 0)[0]
        self.idx_1 = np.where(y == 1)[0]
        self.expanded = np.concatenate([self.idx_1, self.idx_1, self.idx_1], axis=0)
        self.batch_size, self.strategy = int(batch_size), int(strategy)
        self.n = len(y) if n_total is None else int(n_total)
        half = int(batch_size / 2)
        self.n_batches = {1: 10, 3: 30}.get(self.strategy) if self.strategy != 2 else \
            int(np.min([len(self.idx_0) // half, len(self.expanded) // half]))
        if self.strategy not in (1, 2, 3):
            raise ValueError("strategy must be 1, 2 or 3")

    def next_epoch(self):
        half = int(self.batch_size / 2)
        if self.strategy == 2:
            np.random.shuffle(self.expanded)                     # in place, cumulative over epochs (Raindrop.py:293-296)
            np.random.shuffle(self.idx_0)
            return [np.concatenate([self.idx_0[n * half:(n + 1) * half], self.expanded[n * half:(n + 1) * half]], axis=0)
                    for n in range(self.n_batches)]
        if self.strategy == 3:
            return [np.random.choice(list(range(self.n)), size=self.batch_size, replace=False) for _ in range(30)]
        return [np.concatenate([np.random.choice(self.idx_0, size=half, replace=False),
                                np.random.choice(self.idx_1, size=half, replace=False)], axis=0) for _ in range(10)]


def epoch_index_plan(ytrain, batch_size=128, strategy=2, n_total=None):
    """The batches of the FIRST epoch of a run as the reference draws them (`code/Raindrop.py:262-307`), using the global
    numpy RNG exactly like the script (call `np.random.seed` first for reproducibility).  Later epochs of the script
    shuffle the arrays of the previous epoch in place: use `EpochPlanner` for a multi-epoch run.
      strategy 2 (P12/P19): minority class repeated 3x, both classes shuffled (positives first, then
        negatives -- the order of the two `np.random.shuffle` calls matters), batch n = batch_size/2
        negatives ++ batch_size/2 positives, `min(n0, 3*n1) // (batch_size/2)` batches;
      strategy 3 (PAM): 30 batches of `batch_size` distinct samples (`np.random.choice(..., replace=False)`);
      strategy 1: 10 balanced batches drawn without replacement per class (`utils_rd.random_sample`)."""
    y = np.asarray(ytrain).reshape(-1)
    idx_0 = np.where(y == 0)[0]
    idx_1 = np.where(y == 1)[0]
    half = int(batch_size / 2)
    if strategy == 2:
        expanded = np.concatenate([idx_1, idx_1, idx_1], axis=0)
        n_batches = int(np.min([len(idx_0) // half, len(expanded) // half]))
        np.random.shuffle(expanded)
        np.random.shuffle(idx_0)
        return [np.concatenate([idx_0[n * half:(n + 1) * half], expanded[n * half:(n + 1) * half]], axis=0)
                for n in range(n_batches)]
    if strategy == 3:
        n = len(y) if n_total is None else int(n_total)
        return [np.random.choice(list(range(n)), size=int(batch_size), replace=False) for _ in range(30)]
    if strategy == 1:
        return [np.concatenate([np.random.choice(idx_0, size=half, replace=False),
                                np.random.choice(idx_1, size=half, replace=False)], axis=0) for _ in range(10)]
    raise ValueError("strategy must be 1, 2 or 3")


@torch.no_grad()
def evaluate_chunked(model, ds, chunk=2048):
    """`utils_rd.evaluate_standard` (`code/utils_rd.py:310-320`: the whole split through one forward) as
    contiguous chunks: every stage of the model is per-sample, so the concatenated logits are identical
    (tests/test_gpu_parity.py::test_batch_invariance_at_validation_scale) while the activations stay bounded."""
    was_training = model.training
    model.eval()
    outs = []
    try:
        for lo in range(0, ds.N, chunk):
            hi = min(ds.N, lo + chunk)
            P = ds.P[:, lo:hi].contiguous()
            Ptime = ds.Ptime[:, lo:hi].contiguous()
            Pstatic = None if ds.Pstatic is None else ds.Pstatic[lo:hi].contiguous()
            lengths = torch.sum(Ptime > 0, dim=0)
            out, _, _ = model.forward(P, Pstatic, Ptime, lengths)
            outs.append(out)
    finally:
        model.train(was_training)
    return torch.cat(outs, 0) if outs else torch.empty((0, 0), device=ds.dev)


@torch.no_grad()
def evaluate_sharded(model, ds, chunk=2048, group=None):
    """`utils_rd.evaluate_standard` (`code/utils_rd.py:310-320`) over a process group: rank r runs the
    contiguous shard [r*ceil(N/W), ...) of the split through `evaluate_chunked`'s per-chunk forward and the logits are
    all-gathered (RCCL over xGMI with the nccl backend) into the full [N, C] tensor on every rank -- identical to the
    single-process result because every stage of the model is per-sample.  Without an initialised process group this
    is `evaluate_chunked`."""
    import torch.distributed as dist
    if not dist.is_initialized() or dist.get_world_size(group) == 1:
        return evaluate_chunked(model, ds, chunk)
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    per = (ds.N + world - 1) // world
    lo, hi = min(ds.N, rank * per), min(ds.N, (rank + 1) * per)
    was_training = model.training
    model.eval()
    outs = []
    try:
        for a in range(lo, hi, chunk):
            b = min(hi, a + chunk)
            P = ds.P[:, a:b].contiguous()
            Ptime = ds.Ptime[:, a:b].contiguous()
            Pstatic = None if ds.Pstatic is None else ds.Pstatic[a:b].contiguous()
            out, _, _ = model.forward(P, Pstatic, Ptime, torch.sum(Ptime > 0, dim=0))
            outs.append(out)
    finally:
        model.train(was_training)
    C = int(model.n_classes)
    mine = torch.zeros((per, C), dtype=torch.float32, device=ds.dev)          # equal-sized shards for the collective
    if outs:
        mine[: hi - lo] = torch.cat(outs, 0)
    parts = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(parts, mine, group=group)
    return torch.cat(parts, 0)[: ds.N]


# ------------------------------------------------------------------------------------------------
# evaluation through the captured forward (raindrop_amd/evalstep.py) and validation metrics on the device
# ------------------------------------------------------------------------------------------------

_EVAL_STEPS_MAX = 4       # captured forwards kept per model (each holds a chunk's activations); the oldest goes first


def _eval_step(model, ds, B, save_free=True):
    """The cached `EvalStep` of this model for chunks of B samples of `ds`'s shape (one per distinct chunk size: a split has at
    most two, full chunks and the remainder).  Stale ones -- parameters moved, another arithmetic mode -- are rebuilt."""
    from .evalstep import EvalStep
    import os
    steps = model.__dict__.setdefault("_eval_steps", {})
    key = (int(B), int(ds.T), int(ds.W), int(ds.ds), str(ds.dev), int(_lib.load().rd_get_precision()),
           os.environ.get("RD_TOKEN_PLAN", "1") != "0", bool(getattr(model, "use_beta", False)), bool(getattr(model, "compute_distance", False)),
           bool(save_free))
    step = steps.get(key)
    if step is not None and step._param_ptrs() != step._ptrs:
        step = None
    if step is None:
        steps.pop(key, None)
        while len(steps) >= _EVAL_STEPS_MAX:
            steps.pop(next(iter(steps)))
        f32 = dict(dtype=torch.float32, device=ds.dev)
        batch = dict(src=torch.zeros((ds.T, B, ds.W), **f32), times=torch.zeros((ds.T, B), **f32),
                     lengths=torch.zeros((B,), dtype=torch.int64, device=ds.dev),
                     static=torch.zeros((B, ds.ds), **f32) if ds.Pstatic is not None else None)
        step = steps[key] = EvalStep(model, batch, save_free=save_free)
    return step


def _evaluate_range(model, ds, lo, hi, chunk, out, save_free=True):
    """logits of samples [lo, hi) into out[: hi - lo], chunk by chunk through the cached captured forwards: the data is copied
    into a step's input buffers on the device, lengths are counted there (code/Raindrop.py:317), one graph replay per chunk."""
    if model.static and ds.Pstatic is None:
        raise _lib.RaindropHipError("evaluate_captured: the model has static features, the dataset has none")
    for a in range(lo, hi, chunk):
        b = min(hi, a + chunk)
        step = _eval_step(model, ds, b - a, save_free)
        bt = step.batch
        bt["src"].copy_(ds.P[:, a:b])
        bt["times"].copy_(ds.Ptime[:, a:b])
        if bt["static"] is not None:
            bt["static"].copy_(ds.Pstatic[a:b])
        torch.sum(bt["times"] > 0, dim=0, out=bt["lengths"])
        out[a - lo:b - lo].copy_(step.run())


@torch.no_grad()
def evaluate_captured(model, ds, chunk=2048, group=None, save_free=True):
    """`evaluate_chunked` (and, with a process group, `evaluate_sharded`: contiguous shards, logits all-gathered) with every chunk
    run as ONE hipGraph replay of a cached `raindrop_amd.evalstep.EvalStep` instead of one C-ABI call per operator: same
    contract, same [N, C] logits (bit-identical in the padded layout; on the token plan equal within the plan's documented
    logit bounds, tests/test_eval_step_gpu.py).  Dropout is off and the model's mode is not touched.  No host round trip per
    chunk.  save_free=False: the steps run the training forward with its save-for-backward buffers (A/B; same logits bit for bit).
    torch's gloo backend does not gather device tensors: with a group whose backend is not nccl the gather is staged
    through the host."""
    import torch.distributed as dist
    C = int(model.n_classes)
    if ds.N == 0:
        return torch.empty((0, 0), device=ds.dev)
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        out = torch.empty((ds.N, C), dtype=torch.float32, device=ds.dev)
        _evaluate_range(model, ds, 0, ds.N, int(chunk), out, save_free)
        return out
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    per = (ds.N + world - 1) // world
    lo, hi = min(ds.N, rank * per), min(ds.N, (rank + 1) * per)
    mine = torch.zeros((per, C), dtype=torch.float32, device=ds.dev)          # equal-sized shards for the collective
    _evaluate_range(model, ds, lo, hi, int(chunk), mine, save_free)
    if dist.get_backend(group) == "nccl":
        parts = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(parts, mine, group=group)
        return torch.cat(parts, 0)[: ds.N]
    host = mine.cpu()
    parts = [torch.empty_like(host) for _ in range(world)]
    dist.all_gather(parts, host, group=group)
    return torch.cat(parts, 0)[: ds.N].to(ds.dev)


def check_bootstrap(bootstrap, bootstrap_seed=0, ci=0.95):
    """`validate`'s / `fit`'s bootstrap keywords, refused without a device: bootstrap None or an integer in [1, 4096]
    (metrics.BOOT_R_MAX), bootstrap_seed an integer in [0, 2^64), 0 < ci < 1"""
    from .metrics import BOOT_R_MAX
    if bootstrap is not None and (isinstance(bootstrap, bool) or not isinstance(bootstrap, (int, np.integer))
                                  or not 1 <= bootstrap <= BOOT_R_MAX):
        raise ValueError("bootstrap must be None or an integer in [1, %d] (resamples), got %r" % (BOOT_R_MAX, bootstrap))
    if isinstance(bootstrap_seed, bool) or not isinstance(bootstrap_seed, (int, np.integer)) or not 0 <= bootstrap_seed < 2 ** 64:
        raise ValueError("bootstrap_seed must be an integer in [0, 2^64), got %r" % (bootstrap_seed,))
    if isinstance(ci, bool) or not isinstance(ci, (int, float)) or not 0.0 < ci < 1.0:
        raise ValueError("ci must lie in (0, 1) (0.95: the 2.5th and 97.5th percentiles), got %r" % (ci,))


def check_calibration(calibration, temperature=None):
    """`validate`'s calibration keywords (and `fit`'s bins), refused without a device: calibration None or an integer number of bins
    in [1, 256] (metrics.CALIB_M_MAX); temperature None, "fit" or a positive finite float, and only together with `calibration`"""
    from .metrics import CALIB_M_MAX
    if calibration is not None and (isinstance(calibration, bool) or not isinstance(calibration, (int, np.integer))
                                    or not 1 <= calibration <= CALIB_M_MAX):
        raise ValueError("calibration must be None or an integer in [1, %d] (bins), got %r" % (CALIB_M_MAX, calibration))
    if temperature is None:
        return
    if temperature != "fit" and (isinstance(temperature, (bool, str)) or not isinstance(temperature, (int, float, np.integer, np.floating))
                                 or not 0.0 < float(temperature) < float("inf")):
        raise ValueError("temperature must be None, 'fit' or a positive finite float, got %r" % (temperature,))
    if calibration is None:
        raise ValueError("temperature=%r needs calibration=<bins>: it scales the calibration statistics only" % (temperature,))


@torch.no_grad()
def validate(model, ds, transform="sigmoid", chunk=2048, group=None, save_free=True, class_weight=None, label_smoothing=0.0,
             focal_gamma=None, bootstrap=None, bootstrap_seed=0, ci=0.95, calibration=None, temperature=None):
    """The validation / test block of the reference's loop (`code/Raindrop.py:345-370,385-401`) without leaving the device until
    the end: `evaluate_captured` -> `transform` of the logits with torch ("sigmoid": validation, :349; "softmax": test, :388-389;
    None: the logits) -> `metrics.rank_metrics`, `metrics.confusion` and `rd_softmax_xent` on the TRANSFORMED scores (the
    reference's criterion(sigmoid(out), y), :352; None gives the plain cross entropy of the logits) -> ONE device-to-host copy.
    Ranking equals the reference's only under the same transform: it is the transform that produces the ties.
    Returns Python floats `auroc`, `auprc` (binary: column 1, what roc_auc_score(y, probs[:, 1]) gives; more classes: the
    macro mean of the one-vs-rest values; save_free: as in `evaluate_captured`), `loss`, `accuracy`, `precision`, `recall`, `f1` (macro, over all n_classes classes) and
    numpy arrays `auroc_per_class`, `auprc_per_class`, `confusion` [C, C] (rows = true class).  `ds.y` is required.
    class_weight / label_smoothing (raindrop_amd.step.criterion_values): `loss` is CrossEntropyLoss(weight=class_weight,
    label_smoothing=label_smoothing) of the same scores (`rd_softmax_xent_crit`), the training steps' criterion; no other field
    changes.  focal_gamma (raindrop_amd.step.focal_values; label_smoothing must be 0): `loss` is the focal loss of the same scores
    with these class weights (`rd_softmax_xent_focal`); no other field changes.
    bootstrap=R (1 .. 4096; the split must have at most 16384 samples): `metrics.rank_bootstrap(scores, y, n_boot=R, seed=bootstrap_seed,
    alpha=1 - ci)` on the same scores -- with a `group`, on the gathered scores of every rank, the same seed and so the same
    resamples everywhere -- and the result gains, for the column `auroc` / `auprc` describe (binary: column 1; more classes: the
    macro mean), `auroc_ci`, `auprc_ci` ((lower, upper): the two-sided percentile interval at level `ci`), `auroc_se`, `auprc_se` (the
    bootstrap standard error) and `bootstrap_valid` (the resamples whose AUROC is defined: one without a positive or a negative of
    a column is left out of its interval; the AUPRC is defined on all R), in the same device-to-host copy.  None: the launches and
    the keys as without it.
    calibration=M (1 .. 256 bins; at most 64 classes): `metrics.calibration(logits, y, n_bins=M, temperature=T)` and the result gains
    `ece`, `mce`, `brier`, `nll` and the numpy arrays `reliability` [M, 3] (rows, mean confidence, hit rate of every bin; NaN, NaN for
    an empty one) and `reliability_counts` [M, 2] int64 (rows, hits), in the same copy.  They are ALWAYS statistics of
    softmax(logits / T), whatever `transform` is (the sigmoid of two logits is not a distribution), for the column `auroc` describes:
    binary, column 1 one-vs-rest; more classes, the top label.  temperature: None (T = 1), a float, or "fit":
    `metrics.fit_temperature` on this split's logits (at most 16384 samples; with a `group` the gathered logits, so every rank gets
    the same T), which adds `temperature`, `temperature_status` (0: an interior minimum; include/raindrop_hip.h), `ece_uncalibrated`
    and `nll_uncalibrated` (both at T = 1).  A T fitted and scored on the same split is optimistic: the intended use is "fit" on the
    validation split and that float on the test split.  `temperature` without `calibration` is refused.  None, None: the launches
    and the keys as without them."""
    from . import metrics
    from .step import _spliced, check_focal, criterion_entry, criterion_values, focal_values
    check_bootstrap(bootstrap, bootstrap_seed, ci)
    check_calibration(calibration, temperature)
    if ds.y is None:
        raise _lib.RaindropHipError("validate needs the dataset's labels (DeviceDataset(..., y=...))")
    if transform not in ("sigmoid", "softmax", None):
        raise ValueError("transform must be 'sigmoid', 'softmax' or None")
    if focal_gamma is not None:                                           # refused before the evaluation runs, as the constructors do
        check_focal(label_smoothing, focal_gamma)
        focal_values(class_weight, focal_gamma, model.n_classes)
    logits = evaluate_captured(model, ds, chunk, group, save_free=save_free)
    N, C = logits.shape
    crit = criterion_values(class_weight, label_smoothing, C)
    focal = None if focal_gamma is None else focal_values(class_weight, focal_gamma, C)
    scores = torch.sigmoid(logits) if transform == "sigmoid" else torch.softmax(logits, dim=1) if transform == "softmax" else logits
    scores = scores.contiguous()
    r = metrics.rank_metrics(scores, ds.y)
    cm = metrics.confusion(scores, ds.y)
    loss = torch.empty(1, dtype=torch.float32, device=ds.dev)
    dscores = torch.empty_like(scores)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    suffix, vals = criterion_entry(focal, crit)
    buf = None if vals is None else torch.tensor(vals, dtype=torch.float32, device=ds.dev)
    _lib.call("rd_softmax_xent" + suffix, int(N), int(C), _p(scores), _p(ds.y), *_spliced(buf), _p(loss), _p(dscores), st)
    binary = C == 2
    parts = [r["mean"], loss.double(), r["auroc_per_class"], r["auprc_per_class"], cm.reshape(-1).double()]
    if bootstrap is not None:                              # the (n_valid, mean, deviation, lower, upper) rows of the reported column
        boot = metrics.rank_bootstrap(scores, ds.y, n_boot=int(bootstrap), seed=int(bootstrap_seed), alpha=1.0 - float(ci))
        parts.append(boot["summary"][:, 1 if binary else C, :].reshape(-1))
    at_boot = 3 + 2 * C + C * C                            # where the bootstrap rows start; the calibration follows them
    at_cal = at_boot + (10 if bootstrap is not None else 0)
    if calibration is not None:                            # summary[:4], table, counts [, T, status, ECE and NLL at T = 1]
        M, col = int(calibration), 1 if binary else None
        fitted = metrics.fit_temperature(logits, ds.y) if temperature == "fit" else None
        cal = metrics.calibration(logits, ds.y, n_bins=M, column=col,
                                  temperature=fitted["result"] if fitted is not None else None if temperature is None else float(temperature))
        parts += [cal["summary"][:4], cal["table"].reshape(-1), cal["counts"].reshape(-1).double()]
        if fitted is not None:
            plain = metrics.calibration(logits, ds.y, n_bins=M, column=col)
            parts += [fitted["result"][0:1], fitted["result"][5:6], plain["summary"][0:1], plain["summary"][3:4]]
    packed = torch.cat(parts).cpu().numpy()
    auroc_pc, auprc_pc = packed[3:3 + C].copy(), packed[3 + C:3 + 2 * C].copy()
    cmh = np.rint(packed[3 + 2 * C:3 + 2 * C + C * C]).astype(np.int64).reshape(C, C)             # counts < 2^53: exact in float64
    acc, prec, rec, f1 = metrics.summary_from_confusion(cmh)
    out = {"auroc": float(auroc_pc[1] if binary else packed[0]), "auprc": float(auprc_pc[1] if binary else packed[1]),
           "loss": float(packed[2]), "accuracy": acc, "precision": prec, "recall": rec, "f1": f1,
           "auroc_per_class": auroc_pc, "auprc_per_class": auprc_pc, "confusion": cmh}
    if bootstrap is not None:
        sa, sp = packed[at_boot:at_boot + 5], packed[at_boot + 5:at_boot + 10]
        out.update(auroc_ci=(float(sa[3]), float(sa[4])), auprc_ci=(float(sp[3]), float(sp[4])), auroc_se=float(sa[2]),
                   auprc_se=float(sp[2]), bootstrap_valid=int(sa[0]))
    if calibration is not None:
        k = packed[at_cal:]
        out.update(ece=float(k[0]), mce=float(k[1]), brier=float(k[2]), nll=float(k[3]), reliability=k[4:4 + 3 * M].reshape(M, 3).copy(),
                   reliability_counts=np.rint(k[4 + 3 * M:4 + 5 * M]).astype(np.int64).reshape(M, 2))       # counts < 2^53: exact
        if temperature == "fit":
            f = k[4 + 5 * M:]
            out.update(temperature=float(f[0]), temperature_status=int(f[1]), ece_uncalibrated=float(f[2]), nll_uncalibrated=float(f[3]))
    return out


def validate_ema(model, ds, opt, **kw):
    """`validate(model, ds, **kw)` on the AVERAGED weights of `opt` (raindrop_amd.optim.FlatAdam(ema_decay=...)): the flat
    parameters and their average change places for the duration (`opt.ema_weights()`: two in-place exchanges, rd_swap_f32), and the
    cached captured forwards, which read the parameters by address, are replayed as they are -- no new capture, no copy of the
    model.  The training weights are back, bit for bit, when it returns.  Every keyword of `validate` passes through, `bootstrap`,
    `bootstrap_seed` and `ci` among them: the interval then belongs to the averaged weights; `calibration` and `temperature` likewise."""
    with opt.ema_weights():
        return validate(model, ds, **kw)
