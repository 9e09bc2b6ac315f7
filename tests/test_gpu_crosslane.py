"""The cross-lane primitives of csrc/crosslane.hpp (DPP moves and permlane swaps) against a NumPy restatement of the xor
butterfly they replace: for off = W / 2 .. 1, v[i] = v[i] + v[i ^ off], plain float64 adds in that order.  Every comparison
is of bits, in every lane -- the primitives promise the butterfly's pairing tree, not a tolerance.

The restated maximum orders -0 below +0, as v_max_f64 does whichever operand holds which (the instruction set's
GT_NEG_ZERO); numpy.maximum alone leaves that pair to the operand order."""
import numpy as np
import pytest
import torch

from vggsfm_amd import _lib_selftest as S

pytestmark = pytest.mark.gpu

LANES = np.arange(64)
WIDTHS = {8: S.GROUP_SUM_8, 16: S.GROUP_SUM_16, 32: S.GROUP_SUM_32, 64: S.GROUP_SUM_64}
SENTINEL = -12345.0


def butterfly_sum(x, width):
    """x (..., 64) -> the xor butterfly's sums over aligned groups of `width` lanes, in every lane."""
    v = np.array(x, dtype=np.float64)
    off = width // 2
    while off > 0:
        v = v + v[..., LANES ^ off]
        off //= 2
    return v


def max_f64(a, b):
    m = np.maximum(a, b)
    return np.where(a == b, np.where(np.signbit(a), b, a), m)


def butterfly_max(x):
    v = np.array(x, dtype=np.float64)
    for off in (32, 16, 8, 4, 2, 1):
        v = max_f64(v, v[..., LANES ^ off])
    return v


def reduce_scatter(v):
    """block_sum_scatter's wave part restated: v (64, NV) -> (NV,) sums, value i left in one lane (ba_obs.hpp / crosslane.hpp:
    at the step with offset OFF a lane keeps the low half of its values where its bit OFF is clear, the high half where it
    is set, and adds what its partner sent)."""
    nv = v.shape[1]
    dst = np.full(nv, np.nan)
    written = np.zeros(nv, bool)
    n = np.full(64, nv)
    base = np.zeros(64, int)
    off = 32
    while off > 0:
        cap = v.shape[1]
        h = (cap + 1) // 2
        hi = (LANES & off) != 0
        low = v[:, :h]
        up = np.zeros((64, h))
        up[:, :cap - h] = v[:, h:]
        send = np.where(hi[:, None], low, up)
        keep = np.where(hi[:, None], up, low)
        v = keep + send[LANES ^ off]
        n, base = np.where(hi, np.maximum(n - h, 0), np.minimum(n, h)), base + np.where(hi, h, 0)
        off //= 2
    assert v.shape[1] == 1
    for lane in range(64):
        if n[lane] > 0:
            assert not written[base[lane]]
            dst[base[lane]] = v[lane, 0]
            written[base[lane]] = True
    assert written.all()
    return dst


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def run(waves, skip=None, bcast_src=0, scatter=None):
    """waves (n, 64) -> out (NUM_PRIMS, n, 64) [, scatter sums (n, NV)]; n is padded to whole workgroups of 4 wavefronts."""
    n = waves.shape[0]
    nb = (n + 3) // 4
    x = np.zeros((nb * 4, 64))
    x[:n] = waves
    dev = torch.device("cuda:0")
    t_in = torch.from_numpy(x).to(dev)
    t_out = torch.full((S.NUM_PRIMS, nb * 4, 64), SENTINEL, dtype=torch.float64, device=dev)
    t_skip = None
    if skip is not None:
        words = np.zeros(nb * 4, np.uint64)
        words[:n] = skip
        t_skip = torch.from_numpy(words.view(np.int64)).to(dev)
    t_sin = t_sout = None
    nv = 0
    if scatter is not None:
        nv = scatter.shape[2]
        s = np.zeros((nb * 4, 64, nv))
        s[:n] = scatter
        t_sin = torch.from_numpy(s).to(dev)
        t_sout = torch.full((nb * 4, nv), SENTINEL, dtype=torch.float64, device=dev)
    S.check(S.lib().vggs_crosslane(t_in, t_skip, nb, bcast_src, t_sin, nv, t_out, t_sout, S.stream_ptr()), "vggs_crosslane")
    torch.cuda.synchronize()
    out = t_out.cpu().numpy()[:, :n]
    return out if scatter is None else (out, t_sout.cpu().numpy()[:n])


def cases():
    """(n, 64) wavefronts of inputs: the order of the additions shows in the last bits of most of them."""
    rng = np.random.default_rng(20)
    w = []
    for _ in range(24):                                     # magnitudes spread over 2^-40 .. 2^40, both signs
        w.append(rng.choice([-1.0, 1.0], 64) * rng.uniform(1.0, 2.0, 64) * np.exp2(rng.uniform(-40.0, 40.0, 64)))
    base = np.array([1e16, 1.0, -1e16, 3.0, 1e16, -1.0, -1e16, 0.5])
    for shift in range(8):                                  # cancellation: what survives depends on the pairing
        w.append(np.tile(np.roll(base, shift), 8))
    w.append(np.resize(np.array([1e16, 1.0, -1e16]), 64))
    w.append(rng.permutation(np.resize(np.array([1e16, 1.0, -1e16, 1e-3]), 64)))
    for c in (0.1, 1.0 / 3.0, -2.5, 0.0):                   # all equal
        w.append(np.full(64, c))
    for lane in range(64):                                  # one non-zero lane, at every position
        one = np.zeros(64)
        one[lane] = 1.0 + lane * 2.0 ** -30
        w.append(one)
    # for the maximum: zeros of both signs, ties, all negative
    w.append(np.where(rng.integers(0, 2, 64) == 1, -0.0, 0.0))
    w.append(np.full(64, -0.0))
    for lane in (0, 15, 16, 31, 32, 63):
        z = np.full(64, -0.0)
        z[lane] = 0.0
        w.append(z)
    w.append(np.where(rng.integers(0, 2, 64) == 1, -0.0, -1.0))
    w.append(rng.integers(-3, 4, 64).astype(np.float64))    # many ties
    w.append(-rng.uniform(1.0, 2.0, 64))
    w.append(np.resize(np.array([5.0, -7.0, 5.0, 0.0]), 64))
    return np.stack(w)


@pytest.fixture(scope="module")
def unmasked():
    x = cases()
    return x, run(x)


@pytest.mark.parametrize("width", [8, 16, 32, 64])
def test_group_sum_is_the_xor_butterfly(unmasked, width):
    x, out = unmasked
    want, got = butterfly_sum(x, width), out[WIDTHS[width]]
    bad = np.argwhere(bits(got) != bits(want))
    print(f"\ngroup_sum<{width}>: {len(x)} wavefronts, {len(bad)} lanes differ")
    assert len(bad) == 0, (bad[:8], got[tuple(bad[0])], want[tuple(bad[0])])


def test_wave_sum_and_wave_max(unmasked):
    x, out = unmasked
    assert np.array_equal(bits(out[S.WAVE_SUM]), bits(butterfly_sum(x, 64)))
    want = butterfly_max(x)
    bad = np.argwhere(bits(out[S.WAVE_MAX]) != bits(want))
    assert len(bad) == 0, (bad[:8], out[S.WAVE_MAX][tuple(bad[0])], want[tuple(bad[0])])
    # (what the cases are there for: a -0 maximum, a +0 maximum among -0, a tie)
    assert np.signbit(want).all(axis=1).any() and (want.max(axis=1) == x.max(axis=1)).all()


@pytest.mark.parametrize("src", [0, 17, 32, 63])
def test_wave_bcast(src):
    x = cases()[:8]
    out = run(x, bcast_src=src)
    assert np.array_equal(bits(out[S.WAVE_BCAST]), bits(np.repeat(x[:, src:src + 1], 64, axis=1)))


def test_masked_groups_leave_the_active_ones_unchanged():
    """Every pattern of skipping groups of 8 lanes (bit 8 g of the wavefront's word); the groups of 16 and 32 lanes read
    the bits of their first lanes, so every pattern of theirs occurs as well.  Active groups: the unmasked bits.  Skipping
    groups: nothing asserted."""
    rng = np.random.default_rng(21)
    patterns = np.arange(255, dtype=np.uint64)              # (255 = every group of 8 skips: nothing left to check)
    words = np.zeros(255, np.uint64)
    for g in range(8):
        words |= ((patterns >> np.uint64(g)) & np.uint64(1)) << np.uint64(8 * g)
    x = rng.choice([-1.0, 1.0], (255, 64)) * rng.uniform(1.0, 2.0, (255, 64)) * np.exp2(rng.uniform(-40.0, 40.0, (255, 64)))
    out = run(x, skip=words)
    for width in (8, 16, 32):
        first = LANES & ~(width - 1)
        active = ((words[:, None] >> first[None, :].astype(np.uint64)) & np.uint64(1)) == 0      # (255, 64)
        want, got = butterfly_sum(x, width), out[WIDTHS[width]]
        seen = {tuple(a[::width]) for a in active}
        assert len(seen) == 2 ** (64 // width) - (1 if width == 8 else 0), (width, len(seen))
        bad = np.argwhere((bits(got) != bits(want)) & active)
        print(f"\ngroup_sum<{width}>: {len(seen)} patterns, {int(active.sum())} active lanes, {len(bad)} differ")
        assert len(bad) == 0, (width, bad[:8])
    # the whole-wavefront rows are written by the unmasked wavefront alone
    assert np.array_equal(bits(out[S.WAVE_SUM][0]), bits(butterfly_sum(x[0], 64)))
    assert (out[S.WAVE_SUM][1:] == SENTINEL).all()


@pytest.mark.parametrize("nv", S.SCATTER_VALUES)
def test_reduce_scatter_is_wave_sum_per_value(nv):
    rng = np.random.default_rng(nv)
    n = 6
    v = rng.choice([-1.0, 1.0], (n, 64, nv)) * rng.uniform(1.0, 2.0, (n, 64, nv)) * np.exp2(rng.uniform(-40.0, 40.0, (n, 64, nv)))
    v[1] = np.resize(np.array([1e16, 1.0, -1e16, 3.0, 0.5]), (64, nv))
    v[2] = 0.0
    v[2, np.arange(64), np.arange(64) % nv] = 1.0 + np.arange(64) * 2.0 ** -30
    _, got = run(np.zeros((n, 64)), scatter=v)
    for k in range(n):
        want = reduce_scatter(v[k])
        assert np.array_equal(bits(got[k]), bits(want)), (nv, k)
        # ... whose tree per value is wave_sum's
        assert np.array_equal(bits(want), bits(butterfly_sum(v[k].T, 64)[:, 0])), (nv, k)
