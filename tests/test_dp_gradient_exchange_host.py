"""The data-parallel gradient exchange of fine-tuning (``training/sam_trainer.py``: ``GradientBuckets``, the all-reduce overlapped with
backward, and ``all_reduce_gradients``, the plain form behind ``MSAM_DP_OVERLAP=0``) when the ranks do NOT all give a gradient to the same
parameters: a data-dependent graph.  CPU gloo, worlds 2 and 4, two steps (``zero()`` re-arms the buckets).

Reference: DDP semantics, recomputed here serially in float64 - a rank without a gradient contributes zeros, the sum is divided by the
world size, and only a parameter used on no rank has no gradient.  Every rank must hold the same bits afterwards, and so must the
parameters after an AdamW step.  Collectives are matched by call order: a rank that started its buckets in another order than the others
would average unrelated buckets (equal bucket sizes here, so that shows as wrong values rather than a size error), and one that skipped a
``None`` gradient in the plain form would build a shorter flat buffer than the others (a hang).  So every wait has a time limit and no
worker outlives its test."""
import datetime
import os
import socket
import traceback

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

N = 8                                   # elements per parameter: 32 bytes, all buckets of a case the same size
# Usage kinds: "all" every rank, "r0" rank 0 only, "allbut" every rank but the last, "none" no rank.
# A case lists its parameters in BUCKET order (GradientBuckets fills buckets in reverse registration order) and its bucket size.
CASES = {
    # one parameter per bucket: the incomplete buckets sit between buckets that complete from their hooks
    "between": (["all", "r0", "all", "allbut", "all", "none", "all"], N * 4),
    # two parameters per bucket: the first bucket never completes anywhere (its "none" half), the others complete on some ranks only
    "pairs": (["none", "all", "all", "r0", "allbut", "all", "all", "all"], 2 * N * 4),
}
STEPS = 2
LR, WD = 0.05, 0.01


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _used(kind, rank, world):
    return kind == "all" or (kind == "r0" and rank == 0) or (kind == "allbut" and rank != world - 1)


def _terms(case, i, rank, step, dtype):
    """The coefficients of parameter i's loss term on this rank and step: loss_i = sum(t * p) + sum(u * p^2) / 2, gradient t + u * p."""
    g = torch.Generator().manual_seed(10_000 * step + 100 * rank + i + (0 if case == "between" else 50_000))
    t, u = torch.randn(N, generator=g) * 3, torch.rand(N, generator=g) + 0.5
    return t.to(dtype), u.to(dtype)


def _initial(n_params):
    g = torch.Generator().manual_seed(7)
    return [torch.randn(N, generator=g) for _ in range(n_params)]


def _exchange_worker(rank, world, port, path, q):
    try:
        os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
        from micro_sam_amd.training.sam_trainer import GradientBuckets, all_reduce_gradients
        out = {}
        for case, (kinds, bucket_bytes) in CASES.items():
            # parameters registered in reverse bucket order: bucket k holds kinds[k * per : (k + 1) * per]
            params_b = [torch.nn.Parameter(v.clone()) for v in _initial(len(kinds))]
            registered = list(reversed(params_b))
            opt = torch.optim.AdamW(registered, lr=LR, weight_decay=WD)
            buckets = GradientBuckets(registered, bucket_bytes=bucket_bytes) if path == "overlap" else None
            if buckets is not None:
                assert len(buckets.buckets) == len(kinds) * N * 4 // bucket_bytes
                assert [q_ for b in buckets.buckets for q_ in b["params"]] == params_b
            # every rank uses its parameters in its own order: the hooks complete the buckets in different orders on different ranks
            order = list(range(len(kinds)))
            np.random.default_rng(rank).shuffle(order)
            rec = []
            for step in range(STEPS):
                before = [p.detach().numpy().copy() for p in params_b]
                if buckets is not None:
                    buckets.zero()
                else:
                    opt.zero_grad(set_to_none=True)
                loss = None
                for i in order:
                    if _used(kinds[i], rank, world):
                        t, u = _terms(case, i, rank, step, torch.float32)
                        li = (t * params_b[i]).sum() + (u * params_b[i] ** 2).sum() / 2
                        loss = li if loss is None else loss + li
                loss.backward()
                nbytes = buckets.finish() if buckets is not None else all_reduce_gradients(registered, bucket_bytes=bucket_bytes)
                grads = [None if p.grad is None else p.grad.detach().numpy().copy() for p in params_b]
                opt.step()
                after = [p.detach().numpy().copy() for p in params_b]
                rec.append((before, grads, after, nbytes))
            if buckets is not None:
                buckets.remove()
            out[case] = rec
        q.put((rank, out, None))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:                                                   # report at once instead of letting the parent wait for its timeout
        q.put((rank, None, traceback.format_exc()))


def _run(target, world, *args, timeout=120):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, world, port, *args, q)) for r in range(world)]
    try:
        for p in procs:
            p.start()
        res = {}
        for _ in range(world):
            rank, out, err = q.get(timeout=timeout)
            assert err is None, f"rank {rank}:\n{err}"
            res[rank] = out
        return res
    finally:
        for p in procs:
            p.join(timeout=30)
        for p in procs:
            if p.is_alive():
                p.terminate()
                p.join(timeout=10)


def _bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("path", ["overlap", "plain"])
@pytest.mark.parametrize("world", [2, 4])
def test_partial_gradients_average_like_ddp_gloo(world, path):
    res = _run(_exchange_worker, world, path)
    for case, (kinds, bucket_bytes) in CASES.items():
        for step in range(STEPS):
            before = res[0][case][step][0]
            for r in range(world):
                assert all(_bits_equal(a, b) for a, b in zip(res[r][case][step][0], before)), (case, step, r)
            # float64 reference: each rank's gradient from the common parameters, zeros where the rank did not use the parameter
            for i, kind in enumerate(kinds):
                p64 = torch.from_numpy(before[i]).double()
                terms, mags = [], []
                for r in range(world):
                    if _used(kind, r, world):
                        t, u = _terms(case, i, r, step, torch.float64)
                        terms.append(t + u * p64)
                        mags.append(t.abs() + (u * p64).abs())
                    else:
                        terms.append(torch.zeros(N, dtype=torch.float64))
                        mags.append(torch.zeros(N, dtype=torch.float64))
                want = (sum(terms) / world).numpy()
                scale = (sum(mags) / world).numpy()
                grads = [res[r][case][step][1][i] for r in range(world)]
                if kind == "none":
                    assert all(g is None for g in grads), (case, step, i)
                    continue
                assert all(g is not None for g in grads), (case, step, i, kind, [g is None for g in grads])
                for r in range(world):
                    assert _bits_equal(grads[r], grads[0]), (case, step, i, kind, r)
                # fp32: a few roundings in each rank's gradient, world - 1 additions, an exact division (world 2 or 4)
                err = np.abs(grads[0].astype(np.float64) - want)
                assert np.all(err <= (world + 4) * 2.0 ** -24 * scale + 1e-30), (case, step, i, kind, grads[0], want)
            after = res[0][case][step][2]
            for r in range(world):
                assert all(_bits_equal(a, b) for a, b in zip(res[r][case][step][2], after)), (case, step, r)
            for i, kind in enumerate(kinds):
                if kind == "none":
                    assert _bits_equal(after[i], before[i]), (case, step, i)        # no gradient anywhere: AdamW leaves it alone
                else:
                    assert not np.array_equal(after[i], before[i]), (case, step, i, kind)
            nbytes = res[0][case][step][3]
            n_reduced = len(kinds) if path == "overlap" else sum(k != "none" for k in kinds)
            assert all(res[r][case][step][3] == nbytes for r in range(world)) and nbytes == n_reduced * N * 4


# ---- SamTrainer: a model whose graph uses one parameter on some ranks only, both exchange paths

def _disks(n=4, size=96, seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:size, 0:size]
    y = np.zeros((size, size), dtype=np.int64)
    for k in range(n):
        cy, cx = 14 + (k // 2) * 44 + rng.integers(0, 6), 14 + (k % 2) * 44 + rng.integers(0, 6)
        y[(yy - cy) ** 2 + (xx - cx) ** 2 < 100] = k + 1
    return y


class _RankDependentStub(torch.nn.Module):
    """TrainableSAM's interface; masks = scale * (a Gaussian bump at the first prompt) + bias, plus ``extra`` * bump on rank 0 only."""

    def __init__(self):
        super().__init__()
        self.scale = torch.nn.Parameter(torch.tensor(1.0))
        self.bias = torch.nn.Parameter(torch.tensor(-2.0))
        self.extra = torch.nn.Parameter(torch.tensor(0.5))
        from micro_sam_amd.transforms import ResizeLongestSide
        self.transform = ResizeLongestSide(96)

    def image_embeddings_oft(self, batched_inputs):
        for b in batched_inputs:
            b["input_size"] = (96, 96)
        return torch.zeros(len(batched_inputs), 1), batched_inputs

    def forward(self, batched_inputs, image_embeddings, multimask_output=False):
        outs = []
        yy, xx = torch.meshgrid(torch.arange(96.0), torch.arange(96.0), indexing="ij")
        for rec in batched_inputs:
            n = rec["point_coords"].shape[0] if "point_coords" in rec else rec["boxes"].shape[0]
            if "point_coords" in rec:
                cx, cy = rec["point_coords"][:, 0, 0], rec["point_coords"][:, 0, 1]
            else:
                cx, cy = rec["boxes"][:, [0, 2]].mean(1), rec["boxes"][:, [1, 3]].mean(1)
            bump = torch.exp(-((yy[None] - cy[:, None, None]) ** 2 + (xx[None] - cx[:, None, None]) ** 2) / 150.0)
            gain = self.scale * 6 + (self.extra if dist.get_rank() == 0 else 0.0)
            c = 3 if multimask_output else 1
            masks = (gain * bump + self.bias)[:, None].repeat(1, c, 1, 1) * torch.linspace(1.0, 0.8, c)[None, :, None, None]
            low = torch.nn.functional.interpolate(masks, (256, 256), mode="bilinear")
            outs.append({"low_res_masks": low, "masks": masks, "iou_predictions": torch.sigmoid(self.bias).expand(n, c) * 0 + 0.5})
        return outs


def _trainer_worker(rank, world, port, overlap, q):
    try:
        os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
        os.environ["MSAM_DP_OVERLAP"] = overlap
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
        import random
        from micro_sam_amd.training import ConvertToSamInputs, SamTrainer
        torch.manual_seed(0)
        model = _RankDependentStub()                                    # the same initial parameters on every rank
        np.random.seed(10 + rank); random.seed(10 + rank)               # every rank its own prompts
        opt = torch.optim.AdamW(model.parameters(), lr=5e-2)
        tr = SamTrainer(model, opt, ConvertToSamInputs(transform=None), n_sub_iteration=2, n_objects_per_batch=3, mask_prob=0.5,
                        device="cpu")
        y = torch.as_tensor(np.stack([_disks(seed=s + 3 * rank) for s in (0, 1)]))[:, None]
        x = torch.zeros(2, 3, 96, 96)
        extra0 = model.extra.detach().clone()
        hist = tr.fit(3, [(x, y)])
        q.put((rank, ([p.detach().numpy().copy() for p in model.parameters()], [h["allreduce_bytes"] for h in hist],
                      bool(torch.equal(model.extra.detach(), extra0))), None))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        q.put((rank, None, traceback.format_exc()))


@pytest.mark.parametrize("overlap", ["1", "0"])
def test_trainer_replicas_stay_identical_with_a_rank_dependent_graph_gloo(overlap):
    world = 2
    res = _run(_trainer_worker, world, overlap)
    params0, nbytes0, _ = res[0]
    for r in range(world):
        params, nbytes, extra_unchanged = res[r]
        assert all(_bits_equal(a, b) for a, b in zip(params, params0)), (r, params, params0)
        assert nbytes == nbytes0 == [3 * 4] * 3
        assert not extra_unchanged                                       # rank 1 applies the averaged gradient of `extra` too
