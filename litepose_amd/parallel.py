"""Multi-GPU: one process per GPU, images sharded, ONE all-gather of keypoint records.

The path shards trivially (no cross-image op: BN is folded, grouping is per image,
SURVEY.md section 8e).  Each rank runs ``PoseEngine.infer_batch`` on its contiguous slice
and the fixed-capacity records {count, kpts[pcap,J,3+T], scores[pcap]} are exchanged
with a single ``all_gather_into_tensor`` (backend "nccl" == RCCL over xGMI on ROCm;
"gloo" in the CPU tests).  ~8.5 KB/image at pcap 30: latency-bound, so one collective per
batch and no bucketing.  The reference has no counterpart (valid.py:165 DataParallel,
batch 1).

Training shards a step the same way (``core.trainer.do_train(group=...)``): every rank takes its slice of
each batch, the BatchNorms exchange one fp64 row per pass (``all_gather_rows``), ``GradBucket`` averages the gradients
with one all-reduce of one flat buffer and ``broadcast_state`` makes the ranks start equal -- what the reference's
``DistributedDataParallel`` and ``SyncBatchNorm`` do (dist_train.py:255-290).
"""
import torch
import torch.distributed as dist


def shard_range(n_total, rank, world_size):
    """Contiguous split; the first n_total % world ranks get one extra image."""
    base, rem = divmod(n_total, world_size)
    start = rank * base + min(rank, rem)
    return start, start + base + (1 if rank < rem else 0)


def pack_records(kpts, count, scores):
    """-> flat float32 [N, 1 + pcap*J*D + pcap]; count travels bit-cast to float32."""
    N = kpts.shape[0]
    c = count.to(torch.int32).view(N, 1).contiguous().view(torch.float32)
    return torch.cat([c, kpts.reshape(N, -1), scores.reshape(N, -1)], dim=1).contiguous()


def unpack_records(flat, pcap, J, D):
    N = flat.shape[0]
    count = flat[:, :1].contiguous().view(torch.int32).view(N)
    k = pcap * J * D
    kpts = flat[:, 1:1 + k].reshape(N, pcap, J, D)
    scores = flat[:, 1 + k:1 + k + pcap].reshape(N, pcap)
    return kpts, count, scores


def all_gather_records(kpts, count, scores, group=None):
    """Every rank contributes the SAME number of images (pad the last shard); returns the
    records of all ranks in rank order: (kpts [W*N,...], count [W*N], scores [W*N,pcap])."""
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    if world == 1:
        return kpts, count, scores
    N, pcap, J, D = kpts.shape
    flat = pack_records(kpts, count, scores)
    if flat.is_cuda and dist.get_backend(group) == 'gloo':
        # functional check of the N > 1 path on a box without RCCL peers (tests, LP_BENCH_BACKEND=gloo):
        # gloo gathers host buffers
        host = flat.cpu()
        out = torch.empty((world * N, host.shape[1]), dtype=host.dtype)
        dist.all_gather_into_tensor(out, host, group=group)
        return unpack_records(out.to(flat.device), pcap, J, D)
    out = torch.empty((world * N, flat.shape[1]), dtype=flat.dtype, device=flat.device)
    dist.all_gather_into_tensor(out, flat, group=group)
    return unpack_records(out, pcap, J, D)


# ---------------------------------------------------------------------------------- data-parallel training
def group_size(group=None):
    return dist.get_world_size(group) if dist.is_initialized() else 1


def group_rank(group=None):
    return dist.get_rank(group) if dist.is_initialized() else 0


def _via_host(t, group):
    """gloo moves host buffers: a CUDA tensor travels through the host (the functional check of the multi-rank path on a
    box without RCCL peers, as in ``all_gather_records``)."""
    return t.is_cuda and dist.get_backend(group) == 'gloo'


def all_gather_rows(row, group=None):
    """``row`` [L] of every rank -> [W, L] in rank order, the same tensor on every rank; one collective.  A group of one
    (or no process group) gives ``row[None]`` without a collective."""
    world = group_size(group)
    if world == 1:
        return row.reshape(1, -1)
    row = row.contiguous().view(-1)
    if _via_host(row, group):
        host = row.cpu()
        out = torch.empty(world * host.numel(), dtype=host.dtype)
        dist.all_gather_into_tensor(out, host, group=group)
        return out.to(row.device).view(world, -1)
    out = torch.empty(world * row.numel(), dtype=row.dtype, device=row.device)
    dist.all_gather_into_tensor(out, row, group=group)
    return out.view(world, -1)


class GradBucket(object):
    """The gradients of ``params`` (those that require one) as views of ONE flat fp32 buffer, so that a step needs one
    collective: ``zero_grad()`` zeroes the buffer in one launch and points every ``p.grad`` at its view (autograd
    accumulates into an existing ``.grad`` in place), ``all_reduce_mean()`` is one ``all_reduce(SUM)`` of the buffer and one
    in-place multiply by ``1 / W``.  Views start at multiples of four floats: every gradient stays 16-byte aligned.
    Every rank adds the same W buffers; whether the sum has the same bits on every rank and in every run is the
    collective's property (gloo's ring here; RCCL's has not been measured)."""

    def __init__(self, params, group=None):
        self.params = [p for p in params if p.requires_grad]
        if not self.params:
            raise ValueError('GradBucket: no parameter requires a gradient')
        dev = self.params[0].device
        if any(p.dtype != torch.float32 or p.device != dev for p in self.params):
            raise ValueError('GradBucket: float32 parameters on one device')
        self.group = group
        self.offsets, n = [], 0
        for p in self.params:
            self.offsets.append(n)
            n += (p.numel() + 3) // 4 * 4
        self.flat = torch.zeros(n, dtype=torch.float32, device=dev)
        self.views = [self.flat[o:o + p.numel()].view(p.shape) for o, p in zip(self.offsets, self.params)]

    def zero_grad(self):
        self.flat.zero_()
        for p, v in zip(self.params, self.views):
            if p.grad is not v:
                p.grad = v

    def all_reduce_mean(self):
        world = group_size(self.group)
        if world == 1:
            return
        if _via_host(self.flat, self.group):
            host = self.flat.cpu()
            dist.all_reduce(host, op=dist.ReduceOp.SUM, group=self.group)
            self.flat.copy_(host)
        else:
            dist.all_reduce(self.flat, op=dist.ReduceOp.SUM, group=self.group)
        self.flat.mul_(1.0 / world)


def broadcast_state(model, src=0, group=None):
    """Every parameter and buffer of ``model`` takes rank ``src``'s value (``src``: the global rank): what
    ``DistributedDataParallel`` does at construction.  One broadcast per dtype, flattened: two for a LitePose (float32, and
    the int64 ``num_batches_tracked``)."""
    if group_size(group) == 1:
        return
    by_dtype = {}
    for t in list(model.parameters()) + list(model.buffers()):
        by_dtype.setdefault(t.dtype, []).append(t.data)
    for dtype in sorted(by_dtype, key=str):
        ts = by_dtype[dtype]
        flat = torch.cat([t.reshape(-1) for t in ts])
        if _via_host(flat, group):
            host = flat.cpu()
            dist.broadcast(host, src, group=group)
            flat = host.to(flat.device)
        else:
            dist.broadcast(flat, src, group=group)
        o = 0
        for t in ts:
            t.copy_(flat[o:o + t.numel()].view(t.shape))
            o += t.numel()
