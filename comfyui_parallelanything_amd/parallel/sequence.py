"""Sequence parallelism for batch-1 video: ring self-attention over token
shards, one process per GPU.

Every other multi-GPU path here splits the batch; a batch of 1 has nothing
to split. Here the *tokens* are split: LayerNorm, the GEMMs, the FFN and the
cross-attention against the (replicated) text context are row-local and run
on a rank's shard as they are. Only self-attention needs every key, and gets
them from a ring: each rank keeps its query shard, the K/V shards travel
round the ring while the previous shard is being multiplied, and the
per-shard results are combined exactly through their log-sum-exp
(ops.attention_bshd_lse, ops.attention_merge).

Process-group mode only (torch.distributed; "nccl" is RCCL on ROCm, gloo on
the CPU with the same call pattern). Out of scope: block masks (so WAN's
frame window), the MMDiT and UNet families, the in-process engine, hipGraph
capture of the ring and Ulysses-style head all-to-all.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch
import torch.distributed as dist

from .. import ops
from .dist import COMM_STATS, DistInfo


# Set to a list to have ring_attention_bshd append, per step with a transfer
# in flight on a GPU, the pair of events around the wait for it: the time
# between them is transfer the attention did not hide
# (scripts/bench_wan_sp.py). None: no events.
EXPOSED_WAIT_EVENTS: Optional[list] = None


def shard_sizes(total: int, parts: int) -> List[int]:
    """Contiguous near-equal split of ``total`` tokens over ``parts`` ranks:
    the first ``total % parts`` ranks hold one more."""
    base, extra = divmod(int(total), int(parts))
    return [base + (1 if r < extra else 0) for r in range(parts)]


def _peers(info: DistInfo, group):
    """Global ranks of this rank's ring successor and predecessor."""
    n = info.world_size
    nxt, prv = (info.rank + 1) % n, (info.rank - 1) % n
    if group is not None:
        ranks = dist.get_process_group_ranks(group)
        return ranks[nxt], ranks[prv]
    return nxt, prv


def ring_attention_bshd(q, k, v, scale, sizes: Sequence[int], info: DistInfo,
                        group=None) -> torch.Tensor:
    """Self-attention of a token-sharded sequence: this rank's q, k, v shard
    [B, S_r, H, D] (strided views allowed, as in ops.attention_bshd) -> the
    rows of attention over ALL ranks' keys that belong to this rank's
    queries, [B, S_r, H, D].

    ``sizes`` lists every rank's shard length (uneven and 0 allowed; the
    same list on every rank; sizes[info.rank] == S_r). N = world_size steps:
    step i multiplies the local q with the K/V shard that started on rank
    (rank - i) mod N, a shard of length 0 contributing lse = -inf, and one
    ops.attention_merge over the N partials ends the call. K and V travel as
    one contiguous [2, B, S_c, H, D] buffer; the send to rank + 1 and the
    receive from rank - 1 for step i + 1 are posted as one
    dist.batch_isend_irecv before step i's attention and waited for after
    it, so the transfer overlaps the compute. COMM_STATS counts the bytes:
    per call a rank sends 2 * B * H * D * elem bytes times the lengths of
    the N - 1 shards it forwards."""
    sizes = [int(s) for s in sizes]
    n = info.world_size
    if len(sizes) != n:
        raise ValueError(f"ring_attention_bshd: {len(sizes)} shard sizes for "
                         f"{n} ranks")
    if not 1 <= n <= ops.ATTN_MERGE_MAX:
        raise ValueError(f"ring_attention_bshd: 1 to {ops.ATTN_MERGE_MAX} "
                         f"ranks (one partial each), got {n}")
    if not (q.dim() == 4 and q.shape[1] == k.shape[1] == v.shape[1]
            == sizes[info.rank]):
        raise ValueError(
            f"ring_attention_bshd: rank {info.rank} holds q/k/v of "
            f"{q.shape[1]}/{k.shape[1]}/{v.shape[1]} tokens, sizes say "
            f"{sizes[info.rank]}")
    B, _, H, D = q.shape
    cur = torch.stack([k, v])               # [2, B, S_r, H, D], contiguous
    send_to, recv_from = _peers(info, group)
    outs, lses = [], []
    for i in range(n):
        reqs, nxt = [], None
        if i + 1 < n:
            nxt = torch.empty((2, B, sizes[(info.rank - i - 1) % n], H, D),
                              dtype=cur.dtype, device=cur.device)
            p2p = []
            if cur.numel() > 0:
                p2p.append(dist.P2POp(dist.isend, cur, send_to, group))
                COMM_STATS.sent(cur)
            if nxt.numel() > 0:
                p2p.append(dist.P2POp(dist.irecv, nxt, recv_from, group))
                COMM_STATS.recvd(nxt)
            if p2p:
                reqs = dist.batch_isend_irecv(p2p)
        o, l = ops.attention_bshd_lse(q, cur[0], cur[1], scale)
        outs.append(o)
        lses.append(l)
        timed = reqs and EXPOSED_WAIT_EVENTS is not None and q.is_cuda
        if timed:
            ev = (torch.cuda.Event(enable_timing=True),
                  torch.cuda.Event(enable_timing=True))
            ev[0].record()
        for w in reqs:
            w.wait()
        if timed:
            ev[1].record()
            EXPOSED_WAIT_EVENTS.append(ev)
        cur = nxt
    return ops.attention_merge(outs, lses)


class _SequenceParallel:
    """What WanDiT.forward consults when sequence parallelism is installed
    (model._seq_parallel): broadcast of the inputs, this rank's token shard,
    the ring as the blocks' self-attention, and the gather of the output."""

    def __init__(self, info: DistInfo, group=None):
        self.info = info
        self.group = group
        self.sizes: List[int] = []

    def _src(self) -> int:
        if self.group is not None:
            return dist.get_process_group_ranks(self.group)[0]
        return 0

    def broadcast(self, *tensors):
        """Rank 0's values of the forward's tensor arguments, on every rank
        (None stays None; shapes and dtypes already agree, since every rank
        runs the same sampler)."""
        if self.info.world_size == 1:
            return tensors
        out = []
        for t in tensors:
            if t is not None:
                # a copy: never write into the caller's tensor; bool travels
                # as bytes
                as_bool = t.dtype == torch.bool
                t = (t.to(torch.uint8) if as_bool else t.clone()).contiguous()
                dist.broadcast(t, self._src(), group=self.group)
                if as_bool:
                    t = t.bool()
            out.append(t)
        return tuple(out)

    def shard(self, tokens, pe):
        """This rank's contiguous slice of tokens [B, S, ...] and of the RoPE
        table pe [S, ...]; remembers the split for attention and gather."""
        self.sizes = shard_sizes(tokens.shape[1], self.info.world_size)
        lo = sum(self.sizes[:self.info.rank])
        hi = lo + self.sizes[self.info.rank]
        return tokens[:, lo:hi], pe[lo:hi]

    def attention(self, q, k, v, scale):
        return ring_attention_bshd(q, k, v, scale, self.sizes, self.info,
                                   self.group)

    def gather(self, rows):
        """All ranks' [B, S_r, C] rows -> [B, S, C], valid on every rank.
        all_gather needs equal shapes: shards are padded to the longest."""
        n = self.info.world_size
        if n == 1:
            return rows
        longest = max(self.sizes)
        B, _, C = rows.shape
        mine = rows.new_zeros((B, longest, C))
        mine[:, :rows.shape[1]] = rows
        parts = [torch.empty_like(mine) for _ in range(n)]
        dist.all_gather(parts, mine, group=self.group)
        return torch.cat([p[:, :s] for p, s in zip(parts, self.sizes)], dim=1)


def install_sequence_parallel(model, info: DistInfo, group=None):
    """Make ``model`` (a WanDiT) run sequence-parallel over the process group:
    its forward broadcasts x, timesteps, context, image_cond and
    attention_mask from rank 0, patchifies, keeps this rank's token shard
    (contiguous, near-equal, the same split on every rank), runs every block
    on the shard with ring_attention_bshd as the self-attention (cross-
    attention, its key mask, the FFN and the head stay local), and
    all-gathers the shards, so the output is valid on every rank and each
    rank's sampler stays in step. Every rank holds the full weights.

    ``self_attn_frame_window`` together with this raises ValueError, here or
    at the forward. Returns the model."""
    from ..models.wan import WanDiT

    if not isinstance(model, WanDiT):
        raise TypeError(f"sequence parallelism covers WanDiT only, got "
                        f"{type(model).__name__}")
    if info.world_size > 1 and not dist.is_initialized():
        raise RuntimeError("install_sequence_parallel needs an initialised "
                           "process group (process-per-GPU mode)")
    if model.cfg.self_attn_frame_window is not None:
        raise ValueError("self_attn_frame_window with sequence parallelism "
                         "is not supported: the ring has no block masks")
    if not 1 <= info.world_size <= ops.ATTN_MERGE_MAX:
        raise ValueError(f"sequence parallelism over 1 to "
                         f"{ops.ATTN_MERGE_MAX} ranks, got {info.world_size}")
    model._seq_parallel = _SequenceParallel(info, group)
    return model


def uninstall_sequence_parallel(model) -> bool:
    """Back to the local forward. True if something was installed."""
    had = getattr(model, "_seq_parallel", None) is not None
    model._seq_parallel = None
    return had
