"""The host reference of the low-precision AdamW step (tests/optim_lowp_ref.py) on its own: Philox4x32-10 against Random123's known answers, the
rounding rule exhaustively over the 65536 draws, and the statistics the GPU tests hold the kernels to (tests/test_optim_lowp_gpu.py imports the
bounds and the set-ups from here), so that the reference alone is shown to stay inside them."""
import numpy as np
import pytest

from tests import optim_lowp_ref as R

# Random123 kat_vectors, philox4x32 10: counter | key -> output
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]

STAT_N = 1 << 20
STAT_FRACTIONS = (1 / 256, 0.3, 0.5, 0.9)
STAT_SIGMAS = 5.0
CHI2_16_BUCKETS_0999 = 37.7          # the 0.999 quantile of chi-square with 15 degrees of freedom
DRIFT_N, DRIFT_STEPS, DRIFT_ULPS = 65536, 64, 1 / 16


def stat_value(f: float) -> np.float32:
    """1 + 2^-7 f: a fraction f of the way from 1.0 to the next bf16 value (f is rounded to the 16 bits below the bf16 mantissa)"""
    return np.float32(1.0 + 2.0 ** -7 * f)


def stat_fraction(f: float) -> float:
    """the exact probability of rounding stat_value(f) up: its low 16 bits / 65536"""
    return float(int(np.array(stat_value(f)).view(np.uint32)) & 0xFFFF) / 65536


def mean_within_bound(rounded_bits, f: float):
    """-> (|mean - value| in sigmas, the bound) for STAT_N roundings of stat_value(f); sigma = 2^-7 sqrt(q (1 - q) / n)"""
    q = stat_fraction(f)
    value = 1.0 + 2.0 ** -7 * q
    sigma = 2.0 ** -7 * (q * (1 - q) / len(rounded_bits)) ** 0.5
    mean = float(R.widen(rounded_bits).astype(np.float64).mean())
    return abs(mean - value) / sigma, STAT_SIGMAS


def chi2_16(r) -> float:
    counts = np.bincount(np.asarray(r) >> 12, minlength=16).astype(np.float64)
    expect = len(r) / 16
    return float(((counts - expect) ** 2 / expect).sum())


def drift_bound_ulps() -> float:
    return STAT_SIGMAS * (DRIFT_STEPS * DRIFT_ULPS * (1 - DRIFT_ULPS) / DRIFT_N) ** 0.5


@pytest.mark.parametrize("ctr,key,out", KAT)
def test_philox_known_answers(ctr, key, out):
    got = R.philox4x32_10(*ctr, *key)
    assert tuple(int(w[0]) for w in got) == out, [hex(int(w[0])) for w in got]


def test_counter_layout_of_the_draws():
    seed, pi, step = 0x0123456789ABCDEF, 7, 3
    e = np.array([0, 1, 2, 3, 2 ** 33 + 5], dtype=np.int64)
    for word in range(3):
        got = R.draws(seed, pi, step, e, word)
        for i, ei in enumerate(e.tolist()):
            w = R.philox4x32_10((ei >> 1) & 0xFFFFFFFF, (ei >> 1) >> 32, pi, step, seed & 0xFFFFFFFF, seed >> 32)[word]
            assert int(got[i]) == (int(w[0]) >> (16 * (ei & 1))) & 0xFFFF
    assert not np.array_equal(R.draws(seed, pi, step, np.arange(64), 0), R.draws(seed, pi, step + 1, np.arange(64), 0))
    assert not np.array_equal(R.draws(seed, pi, step, np.arange(64), 0), R.draws(seed, pi + 1, step, np.arange(64), 0))
    assert not np.array_equal(R.draws(seed, pi, step, np.arange(64), 0), R.draws(seed + 1, pi, step, np.arange(64), 0))
    assert not np.array_equal(R.draws(seed, pi, step, np.arange(64), 0), R.draws(seed, pi, step, np.arange(64), 1))


ALL_DRAWS = np.arange(65536, dtype=np.uint32)


@pytest.mark.parametrize("bits", [0x3F800001, 0x3F808000, 0x3F80FFFF, 0xBF801234, 0x00000001, 0x0000FFFF, 0x80004000, 0x007FFFFF, 0x7F7F0001,
                                  0x7F7FFFFF, 0xFF7F8000, 0x42F6E979])
def test_rounding_rule_over_every_draw(bits):
    x = np.full(65536, bits, dtype=np.uint32).view(np.float32)
    got = R.sr_round(x, ALL_DRAWS).astype(np.uint32)
    down, low = bits >> 16, bits & 0xFFFF
    assert set(np.unique(got).tolist()) <= {down, down + 1}               # one of the two neighbours (away from zero: the magnitude grows)
    assert int((got == down + 1).sum()) == low                            # up for exactly `low` of the 65536 draws
    assert np.array_equal(got == down + 1, ALL_DRAWS >= 65536 - low)
    if bits in (0x7F7FFFFF, 0xFF7F8000):                                  # the top half-ulp can reach Inf, as round-to-nearest does
        assert (down + 1) & 0x7FFF == 0x7F80


@pytest.mark.parametrize("bits", [0x00000000, 0x80000000, 0x3F800000, 0xBF810000, 0x00010000, 0x7F7F0000, 0xFF7F0000, 0x7F800000, 0xFF800000])
def test_grid_values_and_infinities_never_move(bits):
    x = np.full(65536, bits, dtype=np.uint32).view(np.float32)
    assert np.array_equal(R.sr_round(x, ALL_DRAWS), np.full(65536, bits >> 16, dtype=np.uint16))


@pytest.mark.parametrize("bits", [0x7FC00000, 0x7F800001, 0xFFFFFFFF, 0x7F80FFFF, 0xFF8ABCDE])
def test_nan_stays_a_quiet_nan(bits):
    x = np.full(65536, bits, dtype=np.uint32).view(np.float32)
    got = R.sr_round(x, ALL_DRAWS)
    assert np.array_equal(got, np.full(65536, (bits >> 16) | 0x40, dtype=np.uint16)) and np.isnan(R.widen(got)).all()


def test_rne_is_torchs():
    """the round-to-nearest-even of the master arrangement (NaN aside: converters differ in its payload)"""
    import torch
    x = torch.randn(1 << 16, generator=torch.Generator().manual_seed(0))
    x[:8] = torch.tensor([0.0, -0.0, float("inf"), -float("inf"), 1e-40, 1.00390625, 1.01171875, 3.3895e38])
    want = x.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(R.rne(x.numpy()), want)


@pytest.mark.parametrize("step", [1, 2])
def test_reference_statistics(step):
    e = np.arange(STAT_N, dtype=np.int64)
    for word in range(3):
        r = R.draws(12345, 3, step, e, word)
        c = chi2_16(r)
        print(f"step {step} word {word}: chi-square of the draws over 16 buckets {c:.1f} (bound {CHI2_16_BUCKETS_0999})")
        assert c < CHI2_16_BUCKETS_0999
    r = R.draws(12345, 3, step, e, 0)
    for f in STAT_FRACTIONS:
        dev, bound = mean_within_bound(R.sr_round(np.full(STAT_N, stat_value(f)), r), f)
        print(f"step {step} f {f}: mean of the rounded values {dev:.2f} sigma from the value (bound {bound})")
        assert dev <= bound


def test_reference_keeps_sub_ulp_drift():
    """65536 elements at 1.0, 64 steps of +1/16 bf16 ulp, a fresh draw per step: the mean displacement is 4 ulp to within 5 sigma of the mean
    (0.038 ulp); round-to-nearest never leaves 1.0."""
    ulp = np.float32(2.0 ** -7)
    bits_sr = np.full(DRIFT_N, 0x3F80, dtype=np.uint16)
    bits_rne = bits_sr.copy()
    e = np.arange(DRIFT_N, dtype=np.int64)
    for step in range(1, DRIFT_STEPS + 1):
        bits_sr = R.sr_round(R.widen(bits_sr) + np.float32(DRIFT_ULPS) * ulp, R.draws(9, 0, step, e, 0))
        bits_rne = R.rne(R.widen(bits_rne) + np.float32(DRIFT_ULPS) * ulp)
    moved = float(((R.widen(bits_sr).astype(np.float64) - 1.0) / float(ulp)).mean())
    print(f"mean displacement {moved:.4f} ulp (4 expected, bound {drift_bound_ulps():.3f}); round-to-nearest "
          f"{float((R.widen(bits_rne).astype(np.float64) - 1.0).mean()):.1f}")
    assert abs(moved - DRIFT_STEPS * DRIFT_ULPS) <= drift_bound_ulps() and 0.0375 < drift_bound_ulps() < 0.0385
    assert (bits_rne == 0x3F80).all()


def test_step_reference_arrangements():
    """the step restatement itself: the master arrangement is the default optimizer's recurrence (its bf16 param the RNE of its master), the
    fp32-state arrangement differs from it only through the param's rounding, and nothing leaves the float32 / uint16 types"""
    rng = np.random.default_rng(0)
    p0 = R.rne(rng.standard_normal(1000).astype(np.float32) * 0.02)
    kinds = ["master", (False, "bf16"), (False, "f32"), (True, "bf16")]
    ts = {k: R.Tensor(k, p0, param_index=2, seed=5) for k in kinds}
    for s in range(3):
        g = R.widen(R.rne(rng.standard_normal(1000).astype(np.float32)))
        for t in ts.values():
            t.update(g, 1e-3, (0.9, 0.999), 1e-8, 1e-2)
    assert np.array_equal(ts["master"].p, R.rne(ts["master"].master)) and ts["master"].m.dtype == np.float32
    assert ts[(False, "bf16")].master is None and ts[(False, "bf16")].m.dtype == ts[(False, "bf16")].p.dtype == np.uint16
    assert ts[(True, "bf16")].master.dtype == np.float32 and ts[(True, "bf16")].v.dtype == np.uint16
    # three steps of lr 1e-3 (each moves a weight by about 1e-3): a stochastic rounding moves a value by less than one bf16 ulp, so every
    # arrangement stays within 3 ulps of the fp32-master run, + 1 for the bf16 moments (3 updates of 1e-3, each off by about 2^-8 + 2^-9 of
    # itself, against the smallest ulp used, 2^-15). ulp of the larger of the weight before and after, and of 4e-3: weights cross binades
    ref = ts["master"].master.astype(np.float64)
    ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.maximum(np.abs(ref), np.abs(R.widen(p0))), 4e-3))) - 7)
    for k in kinds[1:]:
        err = np.abs(R.widen(ts[k].p).astype(np.float64) - ref) / ulp
        assert float(err.max()) <= 4.0, (k, float(err.max()))
