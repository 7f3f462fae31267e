"""Plain data-parallel support (the reference has no multi-GPU code; BASELINE.json asks for DP only).

One process per GPU (torchrun-style env: RANK / LOCAL_RANK / WORLD_SIZE / MASTER_*), backend "nccl" (= RCCL over
xGMI on ROCm) on GPUs, "gloo" in CPU tests.  Sequences are independent, so ranks take disjoint shards of every
epoch's seeded permutation; the only exchange is ONE all-reduce(SUM) of the flat gradient buffer per step -- the
loss is a mean over (B,T), so the sum is averaged by 1/world inside the fused optimizer (gt_step_state.grad_scale).
"""
import os

import torch
import torch.distributed as dist


def init_distributed(backend=None):
    """-> (rank, local_rank, world).  No-op (0,0,1) when WORLD_SIZE is unset or 1."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world == 1:
        return 0, 0, 1
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29500")
    if backend is None:
        backend = "nccl" if torch.cuda.is_available() else "gloo"
    if backend == "nccl":
        torch.cuda.set_device(local)
        dist.init_process_group(backend, device_id=torch.device("cuda", local))
    else:
        dist.init_process_group(backend)
    return rank, local, world


def broadcast_parameters(flat, src=0):
    """Identical replicas at start: rank `src`'s flat parameter buffer to everyone."""
    if dist.is_initialized() and dist.get_world_size() > 1:
        dist.broadcast(flat, src)
    return flat


def allreduce_gradients(flat, average=False):
    """ONE collective over the flat gradient buffer.  average=False leaves the 1/world to the optimizer kernel."""
    if dist.is_initialized() and dist.get_world_size() > 1:
        dist.all_reduce(flat, op=dist.ReduceOp.SUM)
        if average:
            flat /= dist.get_world_size()
    return flat


def allreduce_bucket_async(flat, offset, count):
    """Start the SUM all-reduce of flat[offset:offset+count] (one gradient bucket of gt_grad_buckets) and return its work
    handle (None without a process group); call .wait() before the optimizer reads the buffer.  Issued between the two
    halves of a bucketed backward, the collective runs while the second half computes."""
    if dist.is_initialized() and dist.get_world_size() > 1:
        return dist.all_reduce(flat[offset:offset + count], op=dist.ReduceOp.SUM, async_op=True)
    return None


class ShardedBatchSampler:
    """Replaces DataLoader(shuffle=True) (ref:train.py:156-158) under DP: every rank draws the SAME seeded
    permutation of the epoch and keeps indices rank, rank+world, ...; yields lists of `batch_size` indices.
    Ragged tails are dropped so that every rank runs the same number of steps (collectives stay matched)."""

    def __init__(self, n_items, batch_size, rank=0, world=1, seed=0, drop_last=True):
        self.n, self.bs, self.rank, self.world, self.seed, self.drop_last = n_items, batch_size, rank, world, seed, drop_last
        self.epoch = 0

    def set_epoch(self, epoch):
        self.epoch = epoch

    def __len__(self):
        per_rank = self.n // self.world
        return per_rank // self.bs if self.drop_last else (per_rank + self.bs - 1) // self.bs

    def __iter__(self):
        g = torch.Generator()
        g.manual_seed(self.seed * 1000003 + self.epoch)
        perm = torch.randperm(self.n, generator=g)
        per_rank = self.n // self.world
        mine = perm[self.rank: per_rank * self.world: self.world]
        for i in range(len(self)):
            b = mine[i * self.bs:(i + 1) * self.bs]
            if len(b):
                yield b.tolist()


class DeviceBatchLoader:
    """The input pipeline on the device.  The reference's datasets are two dense fp32 tensors of tens of MB
    (ref:dataset.py:263-264,355-356) fed through DataLoader(shuffle=True, pin_memory=True) (ref:train.py:156-158); at
    0.3 ms per train step the collate + H2D copy of a host DataLoader would be several times the step.  Here both tensors
    live in HBM; every epoch draws the SAME seeded permutation on every rank (the one ShardedBatchSampler draws), a rank
    keeps indices rank, rank+world, ....  Two ways to consume it:
      * ``index_batches()`` -> device index tensors only: train_loop hands them to StepEngine.train_step_indexed, where ONE
        gather launch (gt_gather_batch, part of the step's hipGraph) fills both static step inputs -- no batch tensor is ever
        materialised outside the step (the fast path);
      * iteration -> (x, y, idx) like the reference's dataset (two index_select gathers), for any other consumer.
    Under DP ragged tails are dropped (matched collectives); single-process keeps the last partial batch, as DataLoader's
    default does.
    ``DeviceBatchLoader.infilling(hvo, infill_opts, ...)`` is the form for the symbolic infilling experiments: ONE resident tensor of full
    grooves (N,32,27); the pair is drawn on the device (gt_gather_infill).  Only the grooves that can be paired (infill.infill_eligible) are
    permuted; ``index_batches()`` is as above (train_loop hands the indices to StepEngine.train_step_indexed_infill), iteration yields
    (x, y, idx) drawn with this loader's own step state (the loader's seed, step = batches yielded so far).  With event options
    (infill.as_opts: mode="events") the pool is infill.events_eligible, iteration gathers through gt_gather_infill_events and train_loop
    calls StepEngine.train_step_indexed_infill_events."""

    def __init__(self, x, y, batch_size, device, rank=0, world=1, seed=0):
        x = torch.as_tensor(x, dtype=torch.float32).to(device).contiguous()
        y = torch.as_tensor(y, dtype=torch.float32).to(device).contiguous()
        assert x.shape[0] == y.shape[0]
        self._setup(x, y, batch_size, device, rank, world, seed)

    def _setup(self, x, y, batch_size, device, rank, world, seed, infill_opts=None, pool=None, lib=None):
        """every field of either form.  pool: the indices a permutation draws from (None: all of x); infill_opts / lib: the infilling form"""
        self.x, self.y = x, y
        self.infill_opts, self.pool = infill_opts, pool
        self.n = int(x.shape[0] if pool is None else pool.numel())
        self.bs, self.rank, self.world, self.seed = int(batch_size), rank, world, seed
        self.device, self.epoch = device, 0
        self.batch_size = self.bs
        self._lib, self._state, self._drawn = lib, None, 0      # iteration of the infilling form: its library, device step state, batches drawn

    @classmethod
    def infilling(cls, hvo, infill_opts, batch_size, device, rank=0, world=1, seed=0, lib=None):
        """The loader over ONE tensor of full grooves (N,32,27) plus infill options (anything infill.as_opts takes).  lib: the library
        iteration calls (default: the process-wide HIP library; index_batches() needs none)."""
        from . import infill
        x = torch.as_tensor(hvo, dtype=torch.float32).to(device).contiguous()
        io = infill.as_opts(infill_opts)
        pool = infill.eligible(x, io).cpu()
        if pool.numel() == 0:
            raise ValueError("no groove of the set can be paired with these infill options (none has a removable %s)"
                             % ("hit beside another hit" if infill.is_events(io) else "voice beside another active one"))
        self = cls.__new__(cls)
        self._setup(x, None, batch_size, device, rank, world, seed, io, pool, lib)
        return self

    def set_epoch(self, epoch):
        self.epoch = epoch

    def __len__(self):
        per_rank = self.n // self.world
        return per_rank // self.bs if self.world > 1 else (per_rank + self.bs - 1) // self.bs

    def index_batches(self):
        """The epoch's batches as int64 index tensors on the device (views of ONE permutation copied once per epoch)."""
        g = torch.Generator()
        g.manual_seed(self.seed * 1000003 + self.epoch)
        perm = torch.randperm(self.n, generator=g)                      # host generator: identical on every rank and platform
        if self.pool is not None:
            perm = self.pool[perm]                                      # (infilling: the eligible grooves only)
        per_rank = self.n // self.world
        mine = perm[self.rank: per_rank * self.world: self.world].to(self.device)   # ONE small H2D copy per epoch
        for i in range(len(self)):
            yield mine[i * self.bs:(i + 1) * self.bs]

    def __iter__(self):
        if self.infill_opts is not None:
            from . import infill
            if self._state is None:
                self._state = infill.make_state(self.seed, 0, self.x.device)
            for idx in self.index_batches():
                step = torch.tensor([self._drawn & 0x7FFFFFFF], dtype=torch.int32).view(torch.uint8)
                self._state[8:12].copy_(step, non_blocking=True)          # gt_step_state.step: a fresh draw per batch
                self._drawn += 1
                draw = infill.gather_events if infill.is_events(self.infill_opts) else infill.gather
                x, y, _ = draw(self.x, idx, self.infill_opts, self._state, self._lib)
                yield x, y, idx
            return
        for idx in self.index_batches():
            yield self.x.index_select(0, idx), self.y.index_select(0, idx), idx
