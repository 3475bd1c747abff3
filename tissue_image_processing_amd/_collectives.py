"""What the sharded drivers (movie.py, events.py, seg_archive.py, tiling.py) send between ranks: one record format and the two
variable-length collectives that carry it.  Every exchange is a `fields` tuple of (name, dtype) pairs declared next to its use."""
import numpy as np


def pack_records(records, fields):
    """{key: {name: array-like}} -> one flat int64 array.  Per record: the key, one element count per field, then each field
    converted to its declared dtype, flattened, its raw bytes zero-padded to a multiple of eight and viewed as int64."""
    parts = []
    for key, record in records.items():
        arrays = [np.ascontiguousarray(record[name], dtype).reshape(-1) for name, dtype in fields]
        parts.append(np.array([key] + [a.size for a in arrays], np.int64))
        for a in arrays:
            padded = np.zeros(-(-a.nbytes // 8), np.int64)
            padded.view(np.uint8)[:a.nbytes] = a.view(np.uint8)
            parts.append(padded)
    return np.concatenate(parts) if parts else np.zeros(0, np.int64)


def unpack_records(flat, fields):
    """pack_records undone -> {key: {name: array}}, the keys in the order sent, every array a copy that owns its data."""
    flat = np.ascontiguousarray(flat, np.int64)
    records, pos = {}, 0
    while pos < flat.size:
        key, counts = int(flat[pos]), flat[pos + 1:pos + 1 + len(fields)]
        pos += 1 + len(fields)
        records[key] = {}
        for (name, dtype), count in zip(fields, counts):
            nbytes = int(count) * np.dtype(dtype).itemsize
            words = -(-nbytes // 8)
            records[key][name] = flat[pos:pos + words].view(np.uint8)[:nbytes].view(dtype).copy()
            pos += words
    return records


def gather_varlen(flat, dist, rank, world, device, root=None):
    """gatherv of a flat int64 numpy array whose length differs per rank: the sizes are all-gathered first, then one padded
    all_gather (root=None: the per-rank list of arrays on every rank) or one padded gather to `root` (the list there, None
    elsewhere).  A rank with an empty array takes part like any other.  One process: [flat], `dist` untouched."""
    if world == 1:
        return [flat]
    import torch
    flat = np.asarray(flat, np.int64).ravel()
    n = torch.tensor([flat.size], dtype=torch.int64, device=device)
    sizes = [torch.zeros(1, dtype=torch.int64, device=device) for _ in range(world)]
    dist.all_gather(sizes, n)
    sizes = [int(s.item()) for s in sizes]
    m = max(max(sizes), 1)
    buf = torch.zeros(m, dtype=torch.int64, device=device)
    buf[:flat.size] = torch.from_numpy(flat).to(device)
    receives = root is None or rank == root
    out = [torch.zeros_like(buf) for _ in range(world)] if receives else None
    if root is None:
        dist.all_gather(out, buf)
    else:
        dist.gather(buf, out, dst=root)
    return [o[:s].cpu().numpy() for o, s in zip(out, sizes)] if receives else None


def broadcast_varlen(flat, dist, rank, world, device, src=0):
    """`src`'s flat int64 numpy array on every rank (the others' `flat` is ignored): its size, then the array.  One process:
    flat, `dist` untouched."""
    if world == 1:
        return flat
    import torch
    size = torch.tensor([flat.size if rank == src else 0], dtype=torch.int64, device=device)
    dist.broadcast(size, src=src)
    buf = torch.from_numpy(np.asarray(flat, np.int64).ravel()).to(device) if rank == src \
        else torch.zeros(int(size.item()), dtype=torch.int64, device=device)
    dist.broadcast(buf, src=src)
    return buf.cpu().numpy()
