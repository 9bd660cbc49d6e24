"""The contract of a lane backend, primitive by primitive.

Every solve kernel is the same lane-generic code compiled on csrc/lane_gpu.hpp (LaneGpu, LaneBlock, lane_pair.hpp on top) for
the device and on csrc/lane_emu.hpp for the CPU suite.  tests/lane_probe compiles ONE probe (probe.hpp) on both: it calls
the primitive an integer selects on in[block][lane][k] and returns out[block][lane][k].

  * CPU part: the twin (the probe on LaneEmu, built at 64 / 128 / 256 lanes) against the contract written out below in
    plain numpy - from the comments of lane_gpu.hpp, not from lane_emu.hpp's loops.  This pins the emulation.
  * GPU part: the device against the twin BIT FOR BIT, on all lanes except those of EXCLUDED (one table, below); the
    primitives without a twin (end_to_mid, mid_to_end, lane_again .., max_raw_, min_raw_, chain_shift / staged sweeps)
    against numpy; the accuracy figures of rcp_, rsqrt_, rcp_fast_ against exact references.

A failure names the primitive and the backend in the test id."""
import ctypes
import os
import subprocess
import zlib
from fractions import Fraction

import numpy as np
import pytest

import __graft_entry__ as G

K = 20                      # doubles per lane (probe.hpp)
BUILD = os.path.join(G.ROOT, "tests", "_build")

# backend: (id in probe.hpp, kind, lanes per instance, lanes per chain, lanes per block) - as mpmpc_hip.hip instantiates them
BACKENDS = {
    "G64C16": (0, "wave", 64, 16, 64), "G64C32": (1, "wave", 64, 32, 64), "G32C16": (2, "wave", 32, 16, 64),
    "G16C16": (3, "wave", 16, 16, 64), "G64C64": (4, "wave", 64, 64, 64),
    "B128": (5, "block", 128, 64, 128), "B256": (6, "block", 256, 128, 256), "B128CH128": (7, "block", 128, 128, 128),
    "P16": (8, "pair", 16, 16, 64), "P64": (9, "pair", 64, 64, 64), "P128": (10, "pair", 128, 128, 128),
}
BLOCKS = 3


# ------------------------------------------------------------------------------------------------ the two libraries
class Probe:
    """One probe library (same C entry points on the device and on the twin)."""

    def __init__(self, path):
        self.lib = ctypes.CDLL(path)
        self.lib.lane_probe_op_name.restype = ctypes.c_char_p
        dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
        self.lib.lane_probe_run.argtypes = [ctypes.c_int] * 4 + [dp, dp, dp, ctypes.c_int, ip, ctypes.c_int]
        self.ops = {self.lib.lane_probe_op_name(i).decode(): i for i in range(self.lib.lane_probe_op_count())}

    def run(self, be, op, x, arg=0, mem=None, imem=None):
        """x: (blocks, lanes, K) -> out of the same shape; mem (float64) / imem (int32) are updated in place."""
        bid, _, _, _, W = BACKENDS[be]
        assert x.dtype == np.float64 and x.shape[1:] == (W, K) and x.flags.c_contiguous
        assert self.lib.lane_probe_threads(bid) == W, "backend %s is not in this build" % be
        out = np.empty_like(x)
        dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
        m = mem.ctypes.data_as(dp) if mem is not None else None
        im = imem.ctypes.data_as(ip) if imem is not None else None
        rc = self.lib.lane_probe_run(bid, self.ops[op], int(arg), x.shape[0], x.ctypes.data_as(dp), out.ctypes.data_as(dp),
                                     m, 0 if mem is None else mem.size, im, 0 if imem is None else imem.size)
        assert rc == 0, "lane_probe_run(%s, %s, %d) returned %d" % (be, op, arg, rc)
        return out


class Twin:
    def __init__(self):
        self.by_width = {w: Probe(os.path.join(BUILD, "liblaneprobe_emu_w%d.so" % w)) for w in (64, 128, 256)}

    def run(self, be, *a, **kw):
        return self.by_width[BACKENDS[be][4]].run(be, *a, **kw)


@pytest.fixture(scope="module")
def twin():
    """The probe on LaneEmu at 64, 128 and 256 lanes; fails (never skips) when it cannot be built."""
    try:
        subprocess.run(["make", "-s", "-C", os.path.join(G.ROOT, "tests", "emul")] +
                       [os.path.join(BUILD, "liblaneprobe_emu_w%d.so" % w) for w in (64, 128, 256)], check=True)
    except (FileNotFoundError, subprocess.CalledProcessError) as e:
        pytest.fail("the lane probe's twin could not be built: %r" % (e,))
    return Twin()


@pytest.fixture(scope="module")
def device():
    """liblaneprobe.so for gfx950; fails (never skips) when it cannot be built."""
    try:
        return Probe(G.build_lane_probe())
    except (FileNotFoundError, subprocess.CalledProcessError, OSError) as e:
        pytest.fail("liblaneprobe.so could not be built from the tree's sources: %r" % (e,))


def test_build_cross_compiles_the_device_probe():
    """build_lane_probe() needs no GPU: the library exists after it and exports the entry points."""
    so = G.build_lane_probe()
    assert os.path.exists(so) and os.path.basename(so) == "liblaneprobe.so"
    with open(so, "rb") as f:
        blob = f.read()
    assert b"lane_probe_run" in blob and b"gfx950" in blob


# ------------------------------------------------------------------------------------------------ inputs
def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def lane_values(be, nk=3, blocks=BLOCKS):
    """A distinct double on every (block, lane, k): k in the exponent, block and lane in the high dword, a scrambled low dword,
    alternating signs - and one value whose low dword is all zero, one whose high dword is (a DPP move of one half only)."""
    W = BACKENDS[be][4]
    b, i, k = np.meshgrid(np.arange(blocks, dtype=np.uint64), np.arange(W, dtype=np.uint64), np.arange(K, dtype=np.uint64), indexing="ij")
    lo = ((b * np.uint64(7919) + i * np.uint64(K) + k + np.uint64(1)) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)
    lo |= np.uint64(1)
    u = (((b + i + k) & np.uint64(1)) << np.uint64(63)) | ((np.uint64(0x3FF) + k + np.uint64(1)) << np.uint64(52)) | \
        (b << np.uint64(44)) | (i << np.uint64(32)) | lo
    u[0, 5, 0] &= np.uint64(0xFFFFFFFF00000000)
    u[blocks - 1, 9, 1] &= np.uint64(0x00000000FFFFFFFF)
    ks = list(range(nk)) + ([K // 2 + j for j in range(nk)] if BACKENDS[be][1] == "pair" else [])
    x = np.zeros((blocks, W, K))
    x[:, :, ks] = u.view(np.float64)[:, :, ks]
    assert len(np.unique(bits(x[:, :, ks]))) == blocks * W * len(ks)
    return x


def rng_for(*key):
    return np.random.default_rng(zlib.crc32("|".join(str(s) for s in key).encode()))


def wide(rng, shape):
    """Magnitudes over 1e-16 .. 1e16, mixed signs: the order of the additions decides the last bits."""
    return rng.choice([-1.0, 1.0], size=shape) * 10.0 ** rng.uniform(-16, 16, size=shape)


# ------------------------------------------------------------------------------------------------ the contract, in numpy
def move(a, src):
    """a: (blocks, lanes); lane i takes lane src[i] of its block, 0 where src[i] < 0 - a move of BITS."""
    u = bits(a)
    return np.where(src >= 0, u[:, np.clip(src, 0, None)], np.uint64(0)).view(np.float64)


def crosses(C, r):          # lane_gpu.hpp: "the step from the last row of one [wavefront] to the first row of the next crosses"
    return C > 64 and r % 4 == 3


def sources(op, be, arg):
    """Lane exchanges as a source lane per lane (-1: reads 0).  lane_gpu.hpp's comments, backend by backend."""
    _, kind, Gi, C, W = BACKENDS[be]
    i = np.arange(W)
    l, p = i % Gi, i % 16
    if kind == "block" and op in ("mirror", "mirror_n", "cup", "cup_n", "cdown", "cdown_n"):
        C = Gi // 2          # LaneBlock: "lanes [0, G/2) climb, lanes [G/2, G) descend (C = G / 2)" - whatever its CH
    if op in ("up", "up_n", "up1"):
        return np.where(l == 0, -1, i - 1)                                   # "0.0 at the ends of an instance"
    if op in ("down", "down_n", "down1"):
        return np.where(l == Gi - 1, -1, i + 1)
    if op in ("mirror", "mirror_n"):                                         # "the lanes [C, 2C) of an instance are reversed"
        return np.where((l >= C) & (l < 2 * C), i - l + 3 * C - 1 - l, i) if C < Gi else i
    if op in ("cup", "cup_n"):                                               # "lanes 0 and C (cup) .. of an instance read 0"
        if C == Gi:
            return sources("up", be, arg)
        head = l == 0
        if C == 16:
            head |= p == 0                                                   # "chains are rows: the row shift zero-fills" (every row)
        elif (Gi, C) != (64, 32):                                            # "<64,32>: lane 32 .. receives lane 31's value instead of 0"
            head |= l == C
        return np.where(head, -1, i - 1)
    if op in ("cdown", "cdown_n"):                                           # ".. C-1 and 2C-1 (cdown) .."
        if C == Gi:
            return sources("down", be, arg)
        tail = l == Gi - 1
        if C == 16:
            tail |= p == 15
        elif (Gi, C) != (64, 32):                                            # "<64,32>: lane 31 .. receives lane 32's value"
            tail |= l == C - 1
        return np.where(tail, -1, i + 1)
    if op == "rshr":                                                         # "lane i <- lane i - D" inside each row of 16, zero inflow
        return np.where(p >= arg, i - arg, -1)
    if op == "rshl":
        return np.where(p + arg < 16, i + arg, -1)
    if op == "from_even_row":                                                # "a of the same position in the EVEN row of its pair"
        return i & ~16
    if op == "from_odd_row":
        return i | 16
    if op == "from_upper":                                                   # "every lane gets a of lane | 32"
        return i | 32
    if op == "from_lower":                                                   # "a of lane & 31"
        return i & 31
    if op == "bcast15":                                                      # "the lanes of the odd rows get a of lane 15 of the row below .. all others 0"
        return np.where((i & 16) != 0, (i & ~31) | 15, -1)
    if op == "bcast31":                                                      # "lanes 32 .. 63 get a of lane 31 .. all others 0"
        return np.where((i & 32) != 0, 31, -1)
    # Chains of C / 16 rows, in coordinates: lane = 64 wave + 16 row + p, and the lane's row in its chain is (lane % C) // 16.
    # "Inside a wavefront a lane permutation / DPP move per value; the crossing step batches its values through the exchange
    # rows": only the crossing step r moves values between wavefronts.  At every other step pull / push permute the four rows
    # of the wavefront cyclically, down is the wavefront shift (lane 63 reads 0) and bcast is row_bcast:15 "into rows 1 .. 3 of
    # the wavefront" (row 0 reads 0).  A lane without a source in its chain is not part of the contract (EXCLUDED); the twin: 0.
    wave, row = i // 64, (i // 16) % 4
    chain_row, rows = (i % C) // 16, C // 16

    def lane_at(w, r4, pos):
        return 64 * w + 16 * r4 + pos
    if crosses(C, arg):                      # every lane's source is the lane the comment names, in whichever wavefront
        above, below, nxt, last_below = i + 16, i - 16, i + 1, lane_at(wave, row, 0) - 1
        has_next = has_row_below = np.ones(W, bool)
    else:
        above, below = lane_at(wave, (row + 1) % 4, p), lane_at(wave, (row + 3) % 4, p)
        nxt, last_below = i + 1, lane_at(wave, (row + 3) % 4, 15)
        has_next, has_row_below = i % 64 != 63, row != 0
    if op == "cr_pull":                                                      # "v of the same position one row up the chain (lane + 16)"
        return np.where(chain_row + 1 < rows, above, -1)
    if op == "cr_push":                                                      # "one row down (lane - 16)"
        return np.where(chain_row >= 1, below, -1)
    if op == "cr_down":                                                      # "of the next lane"
        return np.where((i % C != C - 1) & has_next, nxt, -1)
    if op == "cr_bcast":                                                     # "of position 15 of the row below"
        return np.where((chain_row >= 1) & has_row_below, last_below, -1)
    raise KeyError(op)


def lane_mask(op, be, arg):
    _, _, Gi, C, W = BACKENDS[be]
    i = np.arange(W)
    p = i % 16
    rung = np.isin(p, (0, 1, 3, 7))                                          # "p = 2^m - 1: 0, 1, 3, 7"
    if op == "cr_elim":                                                      # "eliminated at the .. level of distance D iff p = 15 - D mod 2D"
        return p % (2 * arg) == (15 - arg) % (2 * arg)
    if op == "cr_low15":                                                     # "position 15 of rows 0 and 2"
        return i % 32 == 15
    if op == "cr_special":                                                   # "positions 0, 1, 3, 7 of rows 1, 3"
        return ((i // 16) % 2 == 1) & rung
    # (a wavefront backend counts the rows of the wavefront, "threadIdx.x & 63": "a chain of FOUR rows inside the wavefront")
    chain = max(C, 64)
    if op == "cr64_x":                                                       # "the survivor X of row r (position 15)"
        return i % chain == 16 * arg + 15
    if op == "cr64_special":                                                 # "row r + 1 .. that row's lanes 0, 1, 3, 7"
        return ((i % chain) // 16 == arg + 1) & rung
    raise KeyError(op)


# Lanes whose value is NOT part of the contract - these ops and no others.  (op: excluded(lane, G, C), unit, excluded lanes per
# unit, the line of lane_gpu.hpp that licenses it.)  The twin returns 0 there, the device a wrapped value.
EXCLUDED = {
    "cr_pull": (lambda i, Gi, C: ~((i % C) + 16 < C), "chain", 16,
                "pull: .. one row up the chain (lane + 16) .. (what a lane without such a source gets is not used)"),
    "cr_push": (lambda i, Gi, C: ~((i % C) >= 16), "chain", 16,
                "push: one row down (lane - 16) .. (what a lane without such a source gets is not used)"),
    "cr_down": (lambda i, Gi, C: ~((i % C) != C - 1), "chain", 1,
                "down: of the next lane .. (what a lane without such a source gets is not used)"),
    "cr_bcast": (lambda i, Gi, C: ~((i % C) >= 16), "chain", 16,
                 "bcast: of position 15 of the row below .. (what a lane without such a source gets is not used)"),
    "end_to_mid": (lambda i, Gi, C: i % Gi != C - 1, "instance", None,
                   "lane C - 1 of an instance gets a of its lane 2C - 1 .. What the other lanes get is not used (the caller masks)"),
    "mid_to_end": (lambda i, Gi, C: i % Gi != 2 * C - 1, "instance", None,
                   "lane C - 1 .. gets a of its lane 2C - 1, and back.  What the other lanes get is not used (the caller masks)"),
}


def excluded(op, be):
    _, _, Gi, C, W = BACKENDS[be]
    if op not in EXCLUDED:
        return np.zeros(W, bool)
    return EXCLUDED[op][0](np.arange(W), Gi, C)


# ------------------------------------------------------------------------------------------------ which op on which backend
WAVES = ["G64C16", "G64C32", "G32C16", "G16C16", "G64C64"]
BLOCKB = ["B128", "B256", "B128CH128"]
PAIRS = ["P16", "P64", "P128"]
ALL = WAVES + BLOCKB + PAIRS
ROWED = ["G64C32", "G64C64"] + BLOCKB           # chains of more than one row: on <64,16>, <32,16>, <16,16> no lane has a row above or
#                                                 below it in its chain - cr_pull / cr_push / cr_bcast would compare nothing there

def cr_steps(be):
    return list(range(max(3, BACKENDS[be][3] // 16 - 1)))       # steps r = 0 .. rows - 2 (at CH = 128 that includes the crossing r = 3);
    #                                                             on a wavefront at least the three steps of its four rows


MOVES = {
    "up": ALL, "down": ALL, "up_n": ALL, "down_n": ALL,
    "mirror": ALL, "cup": ALL, "cdown": ALL, "mirror_n": ALL, "cup_n": ALL, "cdown_n": ALL,
    "rshr": WAVES + BLOCKB, "rshl": WAVES + BLOCKB,
    "from_even_row": WAVES, "from_odd_row": WAVES, "from_upper": WAVES, "from_lower": WAVES, "bcast15": WAVES, "bcast31": WAVES,
    "cr_pull": ROWED, "cr_push": ROWED, "cr_down": WAVES + BLOCKB, "cr_bcast": ROWED,
    "up1": PAIRS, "down1": PAIRS,
}
MASKS = {"cr_elim": WAVES + BLOCKB, "cr_low15": WAVES, "cr_special": WAVES, "cr64_x": WAVES + BLOCKB, "cr64_special": WAVES + BLOCKB}
OTHER = {"ids": ALL, "cold": ALL, "load": ALL, "gather": ALL, "loadi": ALL, "gatheri": ALL, "store": ALL, "storei": ALL}
REDUCE = {"gsum": ALL, "gmax": ALL, "gmin": ALL, "gscan": ALL, "gany": ALL, "gcount": ALL, "wany": ALL}


def args_of(op, be):
    if op in ("rshr", "rshl", "cr_elim"):
        return [1, 2, 4, 8]
    if op in ("cr_pull", "cr_push", "cr_down", "cr_bcast", "cr64_x", "cr64_special"):
        return cr_steps(be)
    return [0]


def nvals(op):
    return 3 if op.endswith("_n") else (1 if op in MASKS else 2)


def cases(table):
    return [pytest.param(be, op, id="%s-%s" % (op, be)) for op, bes in table.items() for be in bes]


def pair_split(be, a):
    """(blocks, lanes, K) -> (blocks, lanes, K/2, 2): value k of the two stages of a lane (pair layout of the probe)."""
    return np.stack([a[:, :, :K // 2], a[:, :, K // 2:]], axis=-1)


def pair_join(v):
    return np.concatenate([v[..., 0], v[..., 1]], axis=2)


def expected_move(op, be, arg, x):
    """What the contract says `op` returns on x, all lanes (0 where the twin's lanes without a source are)."""
    kind, W = BACKENDS[be][1], BACKENDS[be][4]
    y = np.zeros_like(x)
    n = nvals(op)
    if kind != "pair":
        src = sources(op, be, arg)
        for k in range(n):
            y[:, :, k] = move(x[:, :, k], src)
        return y
    v = pair_split(be, x)
    o = np.zeros_like(v)
    Gi = BACKENDS[be][2]
    if op in ("up1", "down1"):                   # the lanes' own shift underneath, component by component
        src = sources(op, be, arg)
        for k in range(n):
            for c in range(2):
                o[:, :, k, c] = move(v[:, :, k, c], src)
    else:                                        # in STAGE order: stage 2p + c sits on lane p, component c; 2G stages per instance
        j = np.arange(2 * W)
        if op in ("up", "up_n", "cup", "cup_n"):
            src = np.where(j % (2 * Gi) == 0, -1, j - 1)
        elif op in ("down", "down_n", "cdown", "cdown_n"):
            src = np.where(j % (2 * Gi) == 2 * Gi - 1, -1, j + 1)
        else:                                    # "one chain in stage order: the chain layout is the stage layout"
            assert op in ("mirror", "mirror_n")
            src = j
        for k in range(n):
            o[:, :, k, :] = move(v[:, :, k, :].reshape(-1, 2 * W), src).reshape(-1, W, 2)
    return pair_join(o)


def same_bits(got, want, op, be, arg, skip=None, what="twin vs contract"):
    g, w = bits(got), bits(want)
    bad = g != w
    if skip is not None:
        bad[:, skip, :] = False
    if bad.any():
        b, i, k = [int(t[0]) for t in np.nonzero(bad)]
        pytest.fail("%s<%s>(arg %d), %s: %d values differ, first at block %d lane %d k %d: %r (%#018x) != %r (%#018x)" %
                    (op, be, arg, what, bad.sum(), b, i, k, got[b, i, k], g[b, i, k], want[b, i, k], w[b, i, k]))


# ------------------------------------------------------------------------------------------------ CPU: twin against the contract
@pytest.mark.parametrize("be,op", cases(MOVES))
def test_twin_lane_exchange_matches_the_contract(be, op, twin):
    for arg in args_of(op, be):
        x = lane_values(be, nvals(op))
        same_bits(twin.run(be, op, x, arg), expected_move(op, be, arg, x), op, be, arg)


@pytest.mark.parametrize("be,op", cases(MASKS))
def test_twin_lane_roles_match_the_contract(be, op, twin):
    for arg in args_of(op, be):
        x = lane_values(be, 1)
        want = np.zeros_like(x)
        want[:, :, 0] = lane_mask(op, be, arg)
        same_bits(twin.run(be, op, x, arg), want, op, be, arg)


def test_excluded_lane_table_counts():
    """The lanes left out of the device comparison are exactly those of EXCLUDED: 16 (1 for cr_down) per chain, all but
    one per instance at the junction moves - counted once from the predicates and once in closed form."""
    total = closed = 0
    for op, (pred, unit, per, _) in EXCLUDED.items():
        for be in (MOVES[op] if op in MOVES else DEVICE_ONLY[op]):
            _, _, Gi, C, W = BACKENDS[be]
            total += int(excluded(op, be).sum())
            closed += (W // C) * min(per, C) if unit == "chain" else (W // Gi) * (Gi - 1)
    assert total == closed == EXPECTED_EXCLUDED
    for op in list(MOVES) + list(MASKS) + list(OTHER) + list(REDUCE):
        if op not in EXCLUDED:
            assert not any(excluded(op, be).any() for be in ALL)


def ids_expected(be, x, again=False):
    _, kind, Gi, C, W = BACKENDS[be]
    i = np.arange(W)
    y = np.zeros_like(x)
    if kind == "pair":
        y[:, :, 0], y[:, :, K // 2] = i, i
        y[:, :, 1], y[:, :, K // 2 + 1] = 2 * (i % Gi), 2 * (i % Gi) + 1
        y[:, :, 2], y[:, :, K // 2 + 2] = i // Gi, i // Gi
        if again:
            y[:, :, 0], y[:, :, K // 2] = 0, 0      # (LanePair has stage_again / slot_again only)
    else:
        y[:, :, 0], y[:, :, 1], y[:, :, 2] = i, i % Gi, i // Gi
    return y


def memory_case(be, op):
    """Indices inside the buffers only; lanes with ok = false point at canary words.  -> x, mem, imem, expected out / mem / imem."""
    _, kind, Gi, C, W = BACKENDS[be]
    rng = rng_for("mem", be, op)
    ncomp = 2 if kind == "pair" else 1
    n = BLOCKS * W * ncomp
    canaries = 8
    M = 1 + n + canaries                                    # element 0 exists (gather reads it on lanes without a source)
    ok = rng.random(n) < 0.6
    idx = np.where(ok, 1 + rng.permutation(n), 1 + n + np.arange(n) % canaries)
    assert idx.min() >= 1 and idx.max() < M
    val = np.round(wide(rng, n) % 1e6) if op.endswith("i") else wide(rng, n)
    mem = wide(rng, M)
    imem = rng.integers(-2 ** 30, 2 ** 30, size=M).astype(np.int32)
    mem[1 + n:] = np.array([0xDEADBEEFCAFEF00D], dtype=np.uint64).view(np.float64)[0]
    imem[1 + n:] = -559038737
    x = np.zeros((BLOCKS, W, K))
    sh = (BLOCKS, W, ncomp)
    for c in range(ncomp):
        x[:, :, 0 + c * K // 2] = ok.reshape(sh)[:, :, c]
        x[:, :, 1 + c * K // 2] = idx.reshape(sh)[:, :, c]
        x[:, :, 2 + c * K // 2] = val.reshape(sh)[:, :, c]
    y, m2, im2 = np.zeros_like(x), mem.copy(), imem.copy()
    if op in ("load", "gather"):
        r = np.where(ok, mem[idx], -7.5)
    elif op in ("loadi", "gatheri"):
        r = np.where(ok, imem[idx], -7).astype(np.float64)
    elif op == "store":
        m2[idx[ok]] = val[ok]
        r = np.zeros(n)
    else:
        im2[idx[ok]] = val[ok].astype(np.int32)
        r = np.zeros(n)
    for c in range(ncomp):
        y[:, :, c * K // 2] = r.reshape(sh)[:, :, c]
    return x, mem, imem, y, m2, im2


def check_other(lib, be, op, what):
    if op == "ids":
        x = lane_values(be, 1)
        same_bits(lib.run(be, op, x), ids_expected(be, x), op, be, 0, what=what)
    elif op == "cold":                                   # two slots, read back crosswise
        x = lane_values(be, 2)
        want = np.zeros_like(x)
        for h in ([0, K // 2] if BACKENDS[be][1] == "pair" else [0]):
            want[:, :, h], want[:, :, h + 1] = x[:, :, h + 1], x[:, :, h]
        same_bits(lib.run(be, op, x), want, op, be, 0, what=what)
    else:
        x, mem, imem, y, m2, im2 = memory_case(be, op)
        same_bits(lib.run(be, op, x, 0, mem, imem), y, op, be, 0, what=what)
        assert np.array_equal(bits(mem), bits(m2)), "%s<%s>: the double buffer (or a canary) differs" % (op, be)
        assert np.array_equal(imem, im2), "%s<%s>: the int buffer (or a canary) differs" % (op, be)


@pytest.mark.parametrize("be,op", cases(OTHER))
def test_twin_ids_cold_storage_and_memory_match_the_contract(be, op, twin):
    check_other(twin, be, op, "twin vs contract")


# ---- reductions, scans, ballots
def instances(be):
    """-> (lanes per block, values per lane, stages per instance): the values of an instance as out[block, inst, :]."""
    _, kind, Gi, C, W = BACKENDS[be]
    return W, (2 if kind == "pair" else 1), Gi * (2 if kind == "pair" else 1)


def put(be, s):
    """s: (blocks, stages of the block in stage order) -> the probe's x (value 0)."""
    W, nc, _ = instances(be)
    x = np.zeros((s.shape[0], W, K))
    v = s.reshape(s.shape[0], W, nc)
    x[:, :, 0] = v[:, :, 0]
    if nc == 2:
        x[:, :, K // 2] = v[:, :, 1]
    return x


def get(be, y):
    W, nc, _ = instances(be)
    return (np.stack([y[:, :, 0], y[:, :, K // 2]], axis=-1) if nc == 2 else y[:, :, :1]).reshape(y.shape[0], -1)


def reduction_inputs(be, op):
    """-> [(label, stage values (blocks, stages), 'bits' | 'values')]"""
    W, nc, S = instances(be)
    n = W * nc
    rng = rng_for("red", be, op)
    out = []
    if op in ("gany", "gcount", "wany"):
        z = np.zeros((BLOCKS, n))
        full = np.ones((BLOCKS, n))
        only63 = z.copy(); only63[1, 63 * nc + nc - 1] = 1
        first_of_last = z.copy(); first_of_last[BLOCKS - 1, n - S] = 1
        one_each = z.copy()
        for g in range(n // S):
            one_each[:, g * S + (7 * g + 3) % S] = 1
        one_each[0] = 0
        rnd = (rng.random((BLOCKS, n)) < 0.3).astype(float)
        return [(lab, a, "bits") for lab, a in (("empty", z), ("full", full), ("only lane 63", only63),
                                                ("first lane of the last instance", first_of_last), ("one lane per instance", one_each), ("random", rnd))]
    a = wide(rng, (BLOCKS, n))
    out.append(("wide magnitudes", a, "bits"))
    out.append(("integers", np.round(rng.uniform(-2 ** 30, 2 ** 30, (BLOCKS, n))), "bits"))
    # +-inf and the 1e30 "clipped infinity", in different instances (a sum never meets both infinities: the NaN it would
    # give has no bit pattern in the contract)
    c = wide(rng, (BLOCKS, n))
    ninst = BLOCKS * n // S
    for t, v in enumerate((np.inf, -np.inf, 1e30, -1e30)):
        g = t % ninst if op in ("gsum", "gscan") else (t // 2) % ninst
        c.reshape(ninst, S)[g, (11 * t + 5) % S] = v
    out.append(("infinities and 1e30", c, "bits"))
    if op in ("gmax", "gmin"):
        z = np.where(rng.random((BLOCKS, n)) < 0.5, 0.0, -0.0)
        out.append(("+0 against -0", z, "values"))
        lanes = [0, 15, 16, 31, 32, 63] + [w * 64 + e for w in range(1, W // 64) for e in (0, 63)]
        for ln in lanes:
            b = wide(rng, (BLOCKS, n))
            b[0, ln * nc + (ln & 1) * (nc - 1)] = np.nan
            out.append(("NaN on lane %d" % ln, b, "bits"))
    return out


def scan_contract(be, s):
    """lane_gpu.hpp: gscan - "four shifted adds inside the rows of 16, then the total of the row below (G >= 32) and of the half
    below (G = 64)"; LaneBlock: "then the totals of the wavefronts below, added one after the other"; LanePair: "the lane totals
    are scanned across the lanes, the lanes below add to both stages"."""
    _, kind, Gi, C, W = BACKENDS[be]

    def lanes_scan(a):
        a = a.copy()
        i = np.arange(W)
        for d in (1, 2, 4, 8):
            a = a + move(a, np.where(i % 16 >= d, i - d, -1))
        if Gi >= 32:
            a = a + move(a, np.where((i & 16) != 0, (i & ~31) | 15, -1))
        if Gi >= 64:
            a = a + move(a, np.where((i & 32) != 0, (i & ~63) | 31, -1))
        if Gi > 64:
            off = np.zeros_like(a)
            for w in range(1, Gi // 64):
                off[:, 64 * w:] = off[:, 64 * w:] + a[:, 64 * w - 1:64 * w]
            a = a + off
        return a
    if kind != "pair":
        return lanes_scan(s)
    v = s.reshape(s.shape[0], W, 2)
    t = v[:, :, 0] + v[:, :, 1]
    i = np.arange(W)
    below = move(lanes_scan(t), np.where(i % Gi == 0, -1, i - 1))
    return np.stack([below + v[:, :, 0], below + t], axis=-1).reshape(s.shape[0], -1)


def reduction_contract(be, op, s):
    W, nc, S = instances(be)
    _, kind, Gi, _, _ = BACKENDS[be]
    a = s.reshape(s.shape[0], -1, S)
    with np.errstate(all="ignore"):
        if op == "gsum":            # "bit-identical to the xor butterfly"; pairs: "the lane's two stages first"; workgroups: "pairs of waves first"
            t = a if nc == 1 else a.reshape(a.shape[0], a.shape[1], Gi, 2).sum(axis=-1)
            j = np.arange(Gi)
            off = 1
            while off < Gi:
                t = t + t[:, :, j ^ off]
                off *= 2
            r = np.repeat(t, nc, axis=2)
        elif op == "gmax":
            r = np.broadcast_to(np.fmax.reduce(a, axis=2, keepdims=True), a.shape)
        elif op == "gmin":
            r = np.broadcast_to(np.fmin.reduce(a, axis=2, keepdims=True), a.shape)
        elif op == "gscan":
            return scan_contract(be, s)
        elif op == "gany":
            r = np.broadcast_to((a > 0.5).any(axis=2, keepdims=True), a.shape).astype(float)
        elif op == "gcount":
            r = np.broadcast_to((a > 0.5).sum(axis=2, keepdims=True), a.shape).astype(float)
        else:                       # wany: any lane of the execution group (the wavefront, or the workgroup)
            r = np.broadcast_to((a > 0.5).any(axis=(1, 2), keepdims=True), a.shape).astype(float)
    return np.ascontiguousarray(r).reshape(s.shape[0], -1)


def check_reduction(lib, be, op, ref, what):
    """ref(label, s) -> the stage values `op` must give.  Also: uniform over the instance (but for the scan)."""
    W, nc, S = instances(be)
    for label, s, mode in reduction_inputs(be, op):
        y = lib.run(be, op, put(be, s))
        got, want = get(be, y), ref(label, s)
        if op != "gscan":
            g3 = (got if mode == "values" else bits(got)).reshape(got.shape[0], -1, S)      # (+0 == -0: fmax leaves the sign open)
            assert (g3 == g3[:, :, :1]).all(), "%s<%s>, %s: not uniform over the instance (%s)" % (op, be, label, what)
        if mode == "values":
            assert np.array_equal(got, want), "%s<%s>, %s: values differ (%s)" % (op, be, label, what)
        else:
            bad = bits(got) != bits(want)
            assert not bad.any(), "%s<%s>, %s, %s: %d values differ, first at (block, stage) %r: %r != %r" % (
                op, be, label, what, bad.sum(), tuple(int(t[0]) for t in np.nonzero(bad)), got[bad][0], want[bad][0])
        if label == "integers" and op in ("gsum", "gscan"):     # exact data: any order of additions gives THE sum
            a = s.reshape(s.shape[0], -1, S)
            exact = np.cumsum(a, axis=2) if op == "gscan" else np.broadcast_to(a.sum(axis=2, keepdims=True), a.shape)
            assert np.array_equal(got.reshape(a.shape), exact), "%s<%s>: not the sum of the instance's values (%s)" % (op, be, what)
        if label.startswith("NaN"):
            assert not np.isnan(got).any(), "%s<%s>, %s: the NaN came through (%s)" % (op, be, label, what)


@pytest.mark.parametrize("be,op", cases(REDUCE))
def test_twin_reductions_match_the_contract(be, op, twin):
    check_reduction(twin, be, op, lambda label, s: reduction_contract(be, op, s), "twin vs contract")


# ------------------------------------------------------------------------------------------------ GPU: device against the twin
DEVICE_ONLY = {"end_to_mid": ["G64C16", "G64C32", "G32C16"], "mid_to_end": ["G64C16", "G64C32", "G32C16"], "again": ALL}
# (op, backend, lane) triples of EXCLUDED, summed over the backends above: cr_pull / cr_push / cr_bcast 16 per chain and cr_down 1
# per chain - the first three on the 5 backends whose chains have more than one row (2, 1, 2, 2, 1 = 8 chains), cr_down on all 8
# one-stage backends (4, 2, 4, 4, 1, 2, 2, 1 = 20 chains) - and the junction moves all but one lane per instance on <64,16>,
# <64,32>, <32,16> (63 + 63 + 62 lanes each)
EXPECTED_EXCLUDED = 3 * 16 * 8 + 20 + 2 * (63 + 63 + 62)


@pytest.mark.gpu
@pytest.mark.parametrize("be,op", cases(MOVES))
def test_device_lane_exchange_is_the_twins_bit_for_bit(be, op, device, twin):
    for arg in args_of(op, be):
        x = lane_values(be, nvals(op))
        same_bits(device.run(be, op, x, arg), twin.run(be, op, x, arg), op, be, arg, skip=excluded(op, be), what="device vs twin")


@pytest.mark.gpu
@pytest.mark.parametrize("be,op", cases(MASKS))
def test_device_lane_roles_are_the_twins(be, op, device, twin):
    for arg in args_of(op, be):
        x = lane_values(be, 1)
        same_bits(device.run(be, op, x, arg), twin.run(be, op, x, arg), op, be, arg, what="device vs twin")


@pytest.mark.gpu
@pytest.mark.parametrize("be,op", cases(OTHER))
def test_device_ids_cold_storage_and_memory(be, op, device, twin):
    """Against the contract (canaries included) and, bit for bit, against the twin."""
    check_other(device, be, op, "device vs contract")
    if op in ("ids", "cold"):
        x = lane_values(be, 2)
        same_bits(device.run(be, op, x), twin.run(be, op, x), op, be, 0, what="device vs twin")


@pytest.mark.gpu
@pytest.mark.parametrize("be,op", cases(REDUCE))
def test_device_reductions_are_the_twins_bit_for_bit(be, op, device, twin):
    check_reduction(device, be, op, lambda label, s: get(be, twin.run(be, op, put(be, s))), "device vs twin")


@pytest.mark.gpu
@pytest.mark.parametrize("be,op", cases(DEVICE_ONLY))
def test_device_primitives_without_a_twin(be, op, device):
    _, kind, Gi, C, W = BACKENDS[be]
    i = np.arange(W)
    l = i % Gi
    if op == "again":                # lane_again / stage_again / slot_again: the lane's numbers formed anew
        x = lane_values(be, 1)
        same_bits(device.run(be, op, x), ids_expected(be, x, again=True), op, be, 0, what="device vs contract")
        return
    x = lane_values(be, 2)
    # "lane C - 1 of an instance gets a of its lane 2C - 1, and back"
    src = np.where(l == C - 1, i + C, -1) if op == "end_to_mid" else np.where(l == 2 * C - 1, i - C, -1)
    want = np.zeros_like(x)
    for k in range(2):
        want[:, :, k] = move(x[:, :, k], src)
    skip = excluded(op, be)
    assert (~skip).sum() == W // Gi
    same_bits(device.run(be, op, x), want, op, be, 0, skip=skip, what="device vs contract")


# ---- staged sweeps of the 256-lane workgroup
FILLS = [[(65, 128), (66, 100), (100, 127), (127, 65)], [(128, 66), (100, 65), (65, 66), (128, 127)], [(65, 66), (66, 100), (100, 65), (66, 65)]]


def sweep_inputs(fills, width, exact, rng):
    """Chains right-aligned in lanes [0, 128) and [128, 256); lanes without a stage hold a = b = 0 (x starts at 0)."""
    x = np.zeros((len(fills), 256, K))
    for blk, (n0, n1) in enumerate(fills):
        for c, n in enumerate((n0, n1)):
            sl = slice(128 * c + 128 - n, 128 * c + 128)
            if exact:
                x[blk, sl, :width] = rng.choice([-1.0, 1.0], size=(n, width))
                x[blk, sl, width:2 * width] = rng.integers(-2 ** 20 + 1, 2 ** 20, size=(n, width))
            else:
                x[blk, sl, :width] = rng.uniform(-1.2, 1.2, size=(n, width))
                x[blk, sl, width:2 * width] = rng.standard_normal((n, width))
    return x


def sweep_sequential(x, fills, width, direction):
    """x_j = a_j x_(j-1) + b_j along each chain, one stage after the other (exact data: no FMA needed)."""
    y = np.zeros_like(x)
    for blk, (n0, n1) in enumerate(fills):
        for c, n in enumerate((n0, n1)):
            lanes = list(range(128 * c + 128 - n, 128 * c + 128))
            prev = np.zeros(width)
            for ln in (lanes if direction < 0 else lanes[::-1]):
                prev = x[blk, ln, :width] * prev + x[blk, ln, width:2 * width]
                y[blk, ln, :width] = prev
    return y


@pytest.mark.gpu
@pytest.mark.parametrize("direction", [-1, +1], ids=["inward", "outward"])
@pytest.mark.parametrize("nv", [1, 3, 9, "2x4"])
def test_staged_sweep_chain_shift(nv, direction, device, twin):
    """Solver::staged_sweep over LaneBlock<256>::chain_shift (the hand-off between the two wavefronts of a chain) against
    (i) a sequential numpy recurrence on exact data, (ii) the device's lock-step form, (iii) the twin's lock-step form - bitwise.
    nv = "2x4": a step that shifts twice, edge slots OFF = 0 and OFF = NV.
    steps: DIR -1 `last`, DIR +1 `last + 1` - the relation mpmpc_solver_linalg.hpp keeps between its two sweeps - with last =
    the longest chain of the LAUNCH (one number for its four blocks, like the solver's horizon): the lock-step form needs n
    steps for a chain of n stages (the solver's own last may be n - 1, where its junction step finishes the meeting lane -
    the probe has none); further steps recompute final values.  The staged inward sweep does not depend on it (65 + 64
    steps), the staged outward one runs its second wavefront steps - 64 times."""
    two = nv == "2x4"
    width = 8 if two else nv
    d = "in" if direction < 0 else "out"
    staged, lock = ("sweep2_staged_" if two else "sweep_staged_") + d, ("sweep2_lock_" if two else "sweep_lock_") + d
    for f, fills in enumerate(FILLS):
        last = max(max(p) for p in fills)
        arg = ((last if direction < 0 else last + 1) << 4) | (0 if two else nv)
        rng = rng_for("sweep", nv, direction, f)
        xe = sweep_inputs(fills, width, True, rng)
        same_bits(device.run("B256", staged, xe, arg), sweep_sequential(xe, fills, width, direction), staged, "B256", arg,
                  what="chain_shift: device staged vs sequential numpy, fills %r" % (fills,))
        xr = sweep_inputs(fills, width, False, rng)
        got = device.run("B256", staged, xr, arg)
        same_bits(got, device.run("B256", lock, xr, arg), staged, "B256", arg, what="chain_shift: device staged vs device lock-step, fills %r" % (fills,))
        same_bits(got, twin.run("B256", lock, xr, arg), staged, "B256", arg, what="chain_shift: device staged vs twin lock-step, fills %r" % (fills,))


@pytest.mark.parametrize("direction", [-1, +1], ids=["inward", "outward"])
@pytest.mark.parametrize("nv", [1, 3, 9, "2x4"])
def test_twin_lock_step_sweep_is_the_sequential_recurrence(nv, direction, twin):
    """The CPU reference of the hand-off test itself: the twin's lock-step sweep on exact data against sequential numpy."""
    two = nv == "2x4"
    width = 8 if two else nv
    lock = ("sweep2_lock_" if two else "sweep_lock_") + ("in" if direction < 0 else "out")
    for f, fills in enumerate(FILLS):
        last = max(max(p) for p in fills)
        arg = ((last if direction < 0 else last + 1) << 4) | (0 if two else nv)
        xe = sweep_inputs(fills, width, True, rng_for("sweep", nv, direction, f))
        same_bits(twin.run("B256", lock, xe, arg), sweep_sequential(xe, fills, width, direction), lock, "B256", arg)


# ---- numeric primitives
def numeric_values():
    """4 096 values log-uniform over 1e-12 .. 1e30, the powers of two in that range, 1 +- 1 ulp, 2 - 1 ulp, 4 - 1 ulp, 64 mantissas
    around sqrt(2).  No denormals, zeros or infinities."""
    rng = rng_for("numeric")
    v = [10.0 ** rng.uniform(-12, 30, 4096), 2.0 ** np.arange(-39, 100),
         np.array([np.nextafter(1.0, 2.0), np.nextafter(1.0, 0.0), np.nextafter(2.0, 0.0), np.nextafter(4.0, 0.0)]),
         (np.array([np.sqrt(2.0)]).view(np.uint64)[0] + np.arange(-32, 32).astype(np.uint64)).view(np.float64)]
    return np.concatenate(v)


def numeric_run(device, op, cols):
    """cols: equally long 1-D operand arrays -> the op's results.  ONE launch of 4 blocks of 256 lanes (B256)."""
    n = len(cols[0])
    per = K // len(cols)                       # operand j of result k sits at x[k + j * per] (probe.hpp)
    cap = 4 * 256 * per
    assert n <= cap
    x = np.ones((4 * 256, K))
    for j, c in enumerate(cols):
        blockj = np.ones(cap)
        blockj[:n] = c
        x[:, j * per:(j + 1) * per] = blockj.reshape(4 * 256, per)
    y = device.run("B256", op, np.ascontiguousarray(x.reshape(4, 256, K)))
    return y.reshape(4 * 256, K)[:, :per].reshape(-1)[:n]


def ulp_of(ref):
    """One unit in the last place of a double in the binade of ref (ref: longdouble or float)."""
    _, e = np.frexp(np.abs(ref))
    return np.ldexp(np.longdouble(1.0), e - 53)


@pytest.mark.gpu
def test_rcp_is_within_its_stated_ulp(device):
    """lane_gpu.hpp: rcp_ "1.0 ulp" (+ 0.25: the figure comes from a sampled sweep).  Exact: Fraction arithmetic on the returned bits."""
    a = numeric_values()
    a = np.concatenate([a, -a])
    y = numeric_run(device, "rcp", [a])
    worst = Fraction(0)
    for ai, yi in zip(a.tolist(), y.tolist()):
        exact = 1 / Fraction(ai)
        e = int(np.frexp(float(exact))[1])
        while Fraction(2) ** (e - 1) > abs(exact):
            e -= 1
        while Fraction(2) ** e <= abs(exact):
            e += 1
        worst = max(worst, abs(Fraction(yi) - exact) / Fraction(2) ** (e - 53))
    print("rcp_: max error %.4f ulp over %d values" % (float(worst), len(a)))
    assert float(worst) <= 1.0 + 0.25


@pytest.mark.gpu
def test_rsqrt_is_within_its_stated_ulp(device):
    """lane_gpu.hpp: rsqrt_ "1.24 ulp" (+ 0.25).  Reference in np.longdouble (64-bit mantissa: 2^-11 ulp of a double)."""
    assert np.finfo(np.longdouble).nmant == 63
    a = numeric_values()
    y = numeric_run(device, "rsqrt", [a])
    ref = np.longdouble(1.0) / np.sqrt(a.astype(np.longdouble))
    err = np.abs(y.astype(np.longdouble) - ref) / ulp_of(ref)
    print("rsqrt_: max error %.4f ulp over %d values" % (float(err.max()), len(a)))
    assert float(err.max()) <= 1.24 + 0.25


@pytest.mark.gpu
def test_rcp_fast_is_within_its_stated_relative_error(device):
    """lane_gpu.hpp: rcp_fast_ "relative error 5e-8" (+ 1e-8)."""
    assert np.finfo(np.longdouble).nmant == 63
    a = numeric_values()
    a = np.concatenate([a, -a])
    y = numeric_run(device, "rcp_fast", [a])
    rel = np.abs(y.astype(np.longdouble) * a.astype(np.longdouble) - 1)
    print("rcp_fast_: max relative error %.3e over %d values" % (float(rel.max()), len(a)))
    assert float(rel.max()) <= 5e-8 + 1e-8


@pytest.mark.gpu
def test_sqrt_and_fma_are_correctly_rounded(device, twin):
    a = numeric_values()
    assert np.array_equal(bits(numeric_run(device, "sqrt", [a])), bits(np.sqrt(a))), "sqrt_ is not numpy's (correctly rounded) square root"
    rng = rng_for("fma")
    n = 4 * 256 * (K // 3)
    p, q = wide(rng, n), wide(rng, n)
    r = np.where(rng.random(n) < 0.5, -p * q * (1 + rng.uniform(-1e-15, 1e-15, n)), wide(rng, n))     # half of them cancel
    got = numeric_run(device, "fma", [p, q, r])
    x = np.ones((4 * 256, K))
    per = K // 3
    for j, c in enumerate((p, q, r)):
        x[:, j * per:(j + 1) * per] = c.reshape(-1, per)
    want = twin.run("B256", "fma", np.ascontiguousarray(x.reshape(4, 256, K))).reshape(-1, K)[:, :per].reshape(-1)
    assert np.array_equal(bits(got), bits(want)), "fma_ is not the twin's std::fma"
    for j in range(0, n, 97):                       # ... which is the correctly rounded one (exact, on a sample)
        exact = Fraction(float(p[j])) * Fraction(float(q[j])) + Fraction(float(r[j]))
        assert got[j] == float(exact), "fma_(%r, %r, %r)" % (p[j], q[j], r[j])


@pytest.mark.gpu
def test_max_min_and_their_raw_forms(device):
    """max_raw_ / min_raw_ "return the other operand for a NaN", in either position, and equal max_ / min_ on every pair
    without a NaN - apart from the sign of a zero (+0 against -0: values, not bits)."""
    rng = rng_for("maxmin")
    n = 4096
    a, b = wide(rng, n), wide(rng, n)
    sp = np.array([0.0, -0.0, np.inf, -np.inf, 1e30, -1e30, 1.0, -1.0])
    a[:64], b[:64] = np.repeat(sp, 8), np.tile(sp, 8)
    a[64:128] = b[64:128]                                        # equal operands
    zero_pair = (a == 0) & (b == 0)
    res = {op: numeric_run(device, op, [a, b]) for op in ("max", "min", "max_raw", "min_raw")}
    for op, ref in (("max", np.fmax(a, b)), ("min", np.fmin(a, b))):
        assert np.array_equal(res[op], ref) and np.array_equal(bits(res[op])[~zero_pair], bits(ref)[~zero_pair]), op + "_"
        assert np.array_equal(res[op + "_raw"], res[op]), op + "_raw_ differs from " + op + "_"
        assert np.array_equal(bits(res[op + "_raw"])[~zero_pair], bits(res[op])[~zero_pair]), op + "_raw_ differs from " + op + "_"
    nan = np.full(n, np.nan)
    for op in ("max_raw", "min_raw", "max", "min"):
        assert np.array_equal(bits(numeric_run(device, op, [nan, b])), bits(b)), op + "_(NaN, b) is not b"
        assert np.array_equal(bits(numeric_run(device, op, [a, nan])), bits(a)), op + "_(a, NaN) is not a"
