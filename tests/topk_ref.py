"""Plain numpy restatement of the fixed-budget octree refinement (include/monoport_hip.h: mp_octree_select_topk,
mp_recon_topk_batch) on top of oracle.upsample2x and oracle.lattice_points.  The upstream Seg3dTopk is un-vendored
and unpinned, so this IS the definition the kernels of csrc/topk.hip are held to, bit for bit."""
import numpy as np

from oracle import pifu_oracle as oracle


def select_topk(cur, evaluated, k, max_dist=None, balance=0.5):
    """The nodes one level selects: linear indices z r^2 + y r + x (int64, ascending in the key).

    cur [r,r,r] f32: the upsampled volume; evaluated [r,r,r] bool.  u = |cur - balance| in f32; candidates are the
    nodes that are not evaluated, whose u is not NaN and <= max_dist (None / inf: no bound); selected are the
    min(k, #candidates) smallest under (u, linear index)."""
    cur = np.asarray(cur, np.float32)
    u = np.abs(cur - np.float32(balance)).astype(np.float32).reshape(-1)
    cand = ~np.asarray(evaluated, bool).reshape(-1) & ~np.isnan(u)
    if max_dist is not None:
        with np.errstate(invalid="ignore"):
            cand &= u <= np.float32(max_dist)
    idx = np.flatnonzero(cand).astype(np.int64)
    order = np.lexsort((idx, u[idx]))  # primary key u, ties to the smaller linear index
    return idx[order[:max(int(k), 0)]]


def evaluated_image(evaluated_prev):
    """The even-coordinate image of the previous level's evaluated set at r = 2 rp - 1."""
    rp = evaluated_prev.shape[0]
    ev = np.zeros((2 * rp - 1,) * 3, bool)
    ev[::2, ::2, ::2] = evaluated_prev
    return ev


def seg3d_topk(query_func, b_min, b_max, resolutions, num_points, max_dist=None, balance_value=0.5, stats=None):
    """Coarse-to-fine volume [R,R,R] (z,y,x) f32 with a fixed budget per level, or None if level 0 has nothing
    > balance_value.  ``query_func(points[3,N] f32) -> [N] f32``; num_points[l] = budget of level l (entry 0 ignored:
    level 0 evaluates every node); max_dist: None or one bound per level (None / inf entries: no bound); ``stats``
    receives the points queried per level (level 0 first; nothing more is appended when None is returned)."""
    res = [int(r) for r in resolutions]
    if len(num_points) != len(res) or (max_dist is not None and len(max_dist) != len(res)):
        raise ValueError("one budget (and bound) per level")
    for a, b in zip(res[:-1], res[1:]):
        if b != 2 * a - 1:
            raise ValueError("resolutions must follow r -> 2r-1")
    rf, r0 = res[-1], res[0]
    idx = np.stack(np.meshgrid(np.arange(r0), np.arange(r0), np.arange(r0), indexing="ij"), -1).reshape(-1, 3)
    occ = np.asarray(query_func(oracle.lattice_points(idx, (rf - 1) // (r0 - 1), rf, b_min, b_max)),
                     np.float32).reshape(r0, r0, r0)
    if stats is not None:
        stats.append(idx.shape[0])
    if not (occ > np.float32(balance_value)).any():
        return None
    evaluated = np.ones((r0, r0, r0), bool)
    for level in range(1, len(res)):
        r = res[level]
        occ = oracle.upsample2x(occ)
        evaluated = evaluated_image(evaluated)
        sel = select_topk(occ, evaluated, num_points[level], None if max_dist is None else max_dist[level],
                          balance_value)
        if sel.size:
            zyx = np.stack(np.unravel_index(sel, (r, r, r)), -1)
            vals = np.asarray(query_func(oracle.lattice_points(zyx, (rf - 1) // (r - 1), rf, b_min, b_max)), np.float32)
            occ.reshape(-1)[sel] = vals
            evaluated.reshape(-1)[sel] = True
        if stats is not None:
            stats.append(int(sel.size))
    return occ
