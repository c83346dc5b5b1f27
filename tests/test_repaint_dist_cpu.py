r"""RePaintSampler on the N > 1 path on CPU: two gloo processes, each with its slice of the batch, of ``y`` and of ``mask``; every
noise draw (the DDIM step's, ``randn_like(y)``, ``randn_like(x_s)``) goes through ``Sampler._draw_noise``, so the gathered x0
equals the single-process run sample for sample."""

import os
import socket

import torch
import torch.distributed as dist
import torch.multiprocessing as mp


class Toy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.l1, self.l2 = torch.nn.Linear(5, 32), torch.nn.Linear(32, 5)

    def forward(self, x, t, **kw):
        return self.l2(torch.tanh(self.l1(x) + t))


def observation(batch: int = 8):
    g = torch.Generator().manual_seed(3)
    mask = torch.rand(batch, 5, generator=g) < 0.4
    return torch.randn(batch, 5, generator=g) * mask, mask


def make_sampler(y, mask):
    from azula_amd.denoise import KarrasDenoiser
    from azula_amd.guidance import RePaintSampler
    from azula_amd.noise import VPSchedule

    torch.manual_seed(0)
    den = KarrasDenoiser(Toy(), VPSchedule()).eval()
    return RePaintSampler(den, y, mask, iterations=2, eta=0.4, steps=8, silent=True)


def worker(rank, world, port, out_path, batch=8):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from azula_amd.parallel import init_sharded, sample_sharded, shard_range

        y, mask = observation(batch)
        mine = shard_range(batch, rank, world)
        smp = make_sampler(y[mine.start : mine.stop], mask[mine.start : mine.stop])  # the rank's slice, like per-sample kwargs
        torch.manual_seed(1)
        x_local = init_sharded(smp, (batch, 5))
        torch.manual_seed(2)
        x0 = sample_sharded(smp, x_local)
        after = torch.randn(4)
        if rank == 0:
            torch.save((x0, after), out_path)
    finally:
        dist.destroy_process_group()


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_rank_sharded_repaint_equals_single_process(tmp_path):
    out = str(tmp_path / "x0.pt")
    mp.spawn(worker, args=(2, free_port(), out), nprocs=2, join=True)
    x0, after = torch.load(out)
    y, mask = observation()
    smp = make_sampler(y, mask)
    torch.manual_seed(1)
    x1 = smp.init((8, 5))
    torch.manual_seed(2)
    ref = smp(x1)
    assert torch.equal(x0, ref)
    assert torch.equal(after, torch.randn(4))  # the ranks advanced their generators as the single process did
