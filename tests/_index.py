"""References, groupings and ctypes callers of the indexing entries
(math_amd/csrc/index.hip, rev/fun/index_ops.hpp; tests/test_index_ops.py).

The reference is float64 numpy: `u[g - 1]` for the gather, and per destination
the math.fsum of its terms for the sums (`segment_ref`, which also gives the
sum of the terms' absolute values, the scale of the bound).  `plan` restates
to_dev_index's stable counting sort (perm: the rows sorted by destination,
each destination's rows ascending; offs: each destination's range of perm);
a CPU-only test holds it against numpy's stable argsort and bincount.
Indices are 1-based.
"""
import ctypes
import math

import numpy as np

import gen
from _elt import SENTINEL, SMG_ERR_ARG, SMG_OK, TAIL, Buf  # noqa: F401


# ------------------------------------------------------------ references
def plan(g, J):
    """(perm int32, offs int64) of the 1-based indices g into J destinations,
    by the host layer's counting sort."""
    g = np.asarray(g, dtype=np.int64)
    offs = [0] * (J + 1)
    for gi in g:
        offs[gi] += 1
    for j in range(J):
        offs[j + 1] += offs[j]
    at = list(offs[:-1])
    perm = [0] * len(g)
    for i, gi in enumerate(g):
        perm[at[gi - 1]] = i
        at[gi - 1] += 1
    return np.array(perm, dtype=np.int32), np.array(offs, dtype=np.int64)


def plan_numpy(g, J):
    """The same from numpy's stable sort and bincount (large sizes, and the
    check of `plan`)."""
    g = np.asarray(g, dtype=np.int64)
    perm = np.argsort(g, kind="stable").astype(np.int32)
    offs = np.concatenate([[0], np.cumsum(np.bincount(g - 1, minlength=J))]).astype(np.int64)
    return perm, offs


def gather_ref(u, g):
    return np.asarray(u, dtype=np.float64)[np.asarray(g, dtype=np.int64) - 1]


def segment_ref(v, g, J):
    """(sums, sums of absolute values) per destination, each by math.fsum."""
    v = np.asarray(v, dtype=np.float64)
    perm, offs = plan_numpy(g, J)
    s, a = np.zeros(J), np.zeros(J)
    for j in range(J):
        t = v[perm[offs[j]:offs[j + 1]]]
        s[j], a[j] = math.fsum(t), math.fsum(np.abs(t))
    return s, a


# ------------------------------------------------------------ groupings
def shuffled(a, seed):
    """a in the order of a fixed pseudo-random permutation."""
    return np.asarray(a)[np.argsort(gen.u01(seed, len(a)), kind="stable")]


def from_runs(runs):
    """Sorted g from [(destination, rows), ...]."""
    return np.repeat([d for d, _ in runs], [c for _, c in runs]).astype(np.int32)


def groupings(R, T):
    """{name: (g, J)} at R rows: one destination; all distinct in identity,
    reversed and shuffled order; J = 7 with destinations 1, 4 and 7 empty,
    sorted and shuffled; at R = 3T + 5 the skewed ones: singletons, one
    destination of exactly 2T rows that starts at a tile boundary, singletons
    (`skew aligned`); the same one entry earlier, so that it starts one before
    a boundary and ends one before the next but one (`skew shifted`); and one
    of 2T + 2 rows that starts one before a boundary and ends one after
    another (`skew straddling`); each sorted and with its rows shuffled."""
    ident = np.arange(1, R + 1, dtype=np.int32)
    seven = np.sort(np.array([2, 3, 5, 6], dtype=np.int32)[(gen.u01(gen.SEED + 960, R) * 4).astype(np.int64)])
    out = {
        "one": (np.ones(R, dtype=np.int32), 1),
        "identity": (ident, R),
        "reversed": (ident[::-1].copy(), R),
        "distinct shuffled": (shuffled(ident, gen.SEED + 961), R),
        "seven sorted": (seven, 7),
        "seven shuffled": (shuffled(seven, gen.SEED + 962), 7),
    }
    if R == 3 * T + 5:
        for name, before, big in (("skew aligned", T, 2 * T), ("skew shifted", T - 1, 2 * T),
                                  ("skew straddling", T - 1, 2 * T + 2)):
            after = R - before - big
            runs = [(d + 1, 1) for d in range(before)] + [(before + 1, big)] + \
                   [(before + 2 + d, 1) for d in range(after)]
            g = from_runs(runs)
            assert len(g) == R
            J = before + 1 + after
            out[name] = (g, J)
            out[name + ", rows shuffled"] = (shuffled(g, gen.SEED + 963), J)
    return out


# ------------------------------------------------------------ the C entries
class IntBuf:
    """Integers `a` (int32, or int64 for offs) on the device, `shift` bytes
    past a 16-byte boundary (0, 8, or for int32 4)."""

    def __init__(self, ctx, a, dtype=np.int32, shift=0):
        a = np.asarray(a, dtype=dtype)
        item = a.dtype.itemsize
        assert shift % item == 0
        pre = 16 // item + shift // item
        self.base = ctx.put(np.concatenate([np.zeros(pre, dtype=dtype), a, np.zeros(4, dtype=dtype)]))
        assert self.base % 16 == 0
        self.ptr = self.base + item * pre
        assert self.ptr % 16 == shift


def launch_shape(ctx):
    """{threads, tile, map_threads, map_max_blocks, width} (smg_index_launch_shape)."""
    s = (ctypes.c_int * 5)()
    assert ctx.lib.smg_index_launch_shape(ctx.ptr, s) == SMG_OK
    return dict(zip(("threads", "tile", "map_threads", "map_max_blocks", "width"), list(s)))


def gather(ctx, u, g, dst0=None, mis=(False, 0, False)):
    """smg_gather: dst0 None writes (dst starts as sentinels), else accumulates
    into dst0.  mis: (src one double past a 16-byte boundary, g's shift in
    bytes, dst one double past)."""
    R = len(g)
    bu, bg = Buf(ctx, u, mis[0]), IntBuf(ctx, g, shift=mis[1])
    bd = Buf(ctx, np.full(R, SENTINEL) if dst0 is None else dst0, mis[2])
    ctx.call("smg_gather", bu.ptr, bg.ptr, R, 0 if dst0 is None else 1, bd.ptr)
    return bd.read("gather dst")


class SegmentPlan:
    """perm, offs and the workspace of one grouping on the device."""

    def __init__(self, ctx, g, J, shift=0):
        self.ctx, self.R, self.J = ctx, len(g), J
        perm, offs = plan_numpy(g, J)
        self.perm, self.offs = IntBuf(ctx, perm, shift=shift), IntBuf(ctx, offs, dtype=np.int64)
        self.nws = ctx.lib.smg_segment_sum_ws_doubles(self.R, J)
        assert self.nws >= 1

    def run(self, v, out0, accumulate, mis=(False, False)):
        """out after smg_segment_sum(v, accumulate) on out0; the workspace
        starts as sentinels and must not be overstepped."""
        bv, bo = Buf(self.ctx, v, mis[0]), Buf(self.ctx, out0, mis[1])
        ws = Buf(self.ctx, np.full(self.nws, SENTINEL))
        self.ctx.call("smg_segment_sum", bv.ptr, self.perm.ptr, self.offs.ptr, self.R, self.J, int(accumulate), ws.ptr,
                      bo.ptr)
        ws.read("segment_sum ws")
        return bo.read("segment_sum out")
