"""The one variable-length collective of the sharded drivers (movie.py, tiling.py)."""
import numpy as np


def gather_varlen(flat, dtype, dist, rank, world, device, root=None):
    """gatherv of a flat numpy array (dtype np.float64 or np.int64) whose length differs per rank: the sizes are all-gathered
    first, then one padded all_gather (root=None: the per-rank list of arrays on every rank) or one padded gather to `root`
    (the list there, None elsewhere).  A rank with an empty array takes part like any other."""
    import torch
    flat = np.asarray(flat, dtype).ravel()
    n = torch.tensor([flat.size], dtype=torch.int64, device=device)
    sizes = [torch.zeros(1, dtype=torch.int64, device=device) for _ in range(world)]
    dist.all_gather(sizes, n)
    sizes = [int(s.item()) for s in sizes]
    m = max(max(sizes), 1)
    buf = torch.zeros(m, dtype=torch.from_numpy(flat).dtype, device=device)
    buf[:flat.size] = torch.from_numpy(flat).to(device)
    receives = root is None or rank == root
    out = [torch.zeros_like(buf) for _ in range(world)] if receives else None
    if root is None:
        dist.all_gather(out, buf)
    else:
        dist.gather(buf, out, dst=root)
    return [o[:s].cpu().numpy() for o, s in zip(out, sizes)] if receives else None
