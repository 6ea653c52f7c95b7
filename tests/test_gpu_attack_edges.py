"""The attack-stage kernels of csrc/attack_kernels.hip on ragged batches at their edges: the polyphase
resampler at eleven ratios on clips from 1 to 2049 samples, every iir_kernel<NC> (ncoef 2..12) in both modes from scipy's
shortest filtfilt clip to all chunks, Gaussian noise at lengths that are no multiple of the four samples of a Philox block,
PCM and waveform normalisation next to longer and silent clips, segment cuts at both ends of a clip, decimation of clips
shorter than the factor, the phase vocoder at its 3-frame minimum and the spectral quantiser on digitally silent frames.

Every comparison is against a float64 statement of the same operation (scipy, numpy or the oracle) on the same float32
operands; every tolerance is derived from the number formats or inherited from tests/test_gpu_attacks.py, none is tuned.
Each test prints its worst error next to its bound.

Run on the MI355X box:  python -m pytest tests/test_gpu_attack_edges.py -m gpu -q -s"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def A():
    from aware_amd._lib import require_gpu
    require_gpu()
    from aware_amd import attacks
    return attacks


@pytest.fixture(scope="module")
def rt(A):
    from aware_amd import runtime
    return runtime


@pytest.fixture(scope="module")
def O():
    from oracle import aware_oracle
    return aware_oracle


def noise(rng, n):
    return (0.1 * rng.standard_normal(n)).astype(np.float32)


# ---- 1. polyphase resampler ------------------------------------------------------------------------------------------
# (up, down) reduced, and the same ratio as a pair of rates whose gcd resample_poly_batch has to take out
RATIOS = [((2, 1), (16000, 8000)), ((1, 2), (8000, 16000)), ((1, 3), (16000, 48000)), ((3, 1), (48000, 16000)),
          ((2, 3), (32000, 48000)), ((3, 2), (48000, 32000)), ((5, 8), (10000, 16000)), ((320, 441), (32000, 44100)),
          ((147, 160), (44100, 48000)), ((21, 20), (16800, 16000)), ((1, 6), (8000, 48000))]
# neither the longest nor the shortest clip is first or last
UPFIRDN_LENS = [20, 2049, 3, 255, 1, 1000, 7, 41, 2, 1025, 19, 21]


def dot_terms(x64, h64, up, down, half_len, n_out):
    """y[j] = sum_i x[i] h[j*down - i*up + half_len] over the taps that exist, in float64, and the standard bound of the same
    sum carried in float32: (taps in the sum + 1) * 2^-24 * sum_i |x_i h_i| (n products and n - 1 additions, each one
    rounding of at most 2^-24 relative: gamma_n <= n u to first order, one more u for the reference's operands)."""
    n_in, nh = len(x64), len(h64)
    pos = np.arange(n_out, dtype=np.int64) * down + half_len
    k = np.arange((nh - 1) // up + 1, dtype=np.int64)
    idx = (pos // up)[:, None] - k[None, :]
    tap = (pos % up)[:, None] + k[None, :] * up
    ok = (idx >= 0) & (idx < n_in) & (tap < nh)
    prod = np.where(ok, x64[np.clip(idx, 0, n_in - 1)] * h64[np.clip(tap, 0, nh - 1)], 0.0)
    return prod.sum(axis=1), (ok.sum(axis=1) + 1) * 2.0 ** -24 * np.abs(prod).sum(axis=1)


@pytest.mark.parametrize("ratio,rates", RATIOS, ids=[f"{u}_{d}" for (u, d), _ in RATIOS])
def test_upfirdn_ragged_ratios(A, rt, ratio, rates):
    """upfirdn_kernel through attacks.resample_poly_batch: one ragged launch of twelve clips of 1 to 2049 samples per ratio,
    every output sample against scipy.signal.resample_poly in float64 with the kernel's own float32 taps, to the float32
    dot-product bound of dot_terms.  The unreduced rates must give the same bits as the reduced ratio.
    On the CPU a float32 restatement of the kernel's loop and scipy's own float32 path reach 0.20 (320/441) to 0.40 (21/20)
    of the bound on these clips; an output at a clip's edge that meets one tap is one rounding against a bound of two, so
    0.5 is within reach of any correct float32 sum.  Measured on the MI355X: the same, 0.20 to 0.40 per ratio."""
    from scipy import signal
    up, down = ratio
    rng = np.random.default_rng(101)
    clips = [noise(rng, n) for n in UPFIRDN_LENS]
    x = rt.Ragged.from_list(clips)
    got = A.resample_poly_batch(x, up, down).to_list()
    got_unreduced = A.resample_poly_batch(x, rates[0], rates[1]).to_list()
    h32, half = A._resample_filter(up, down, x.data.device)
    h64 = h32.cpu().numpy().astype(np.float64)
    worst = 0.0
    for c, y, yu in zip(clips, got, got_unreduced):
        n_out = -(-len(c) * up // down)
        assert y.shape == (n_out,) and y.dtype == np.float32, (len(c), y.shape)
        np.testing.assert_array_equal(y, yu)
        c64 = c.astype(np.float64)
        ref = signal.resample_poly(c64, up, down, window=h64 / up)
        direct, bound = dot_terms(c64, h64, up, down, half, n_out)
        assert ref.shape == (n_out,) and np.max(np.abs(ref - direct)) <= 1e-14      # scipy sums the same index set
        err = np.abs(y.astype(np.float64) - ref)
        frac = float(np.max(err / np.maximum(bound, 1e-300)))
        worst = max(worst, frac)
        assert np.all(err <= bound), (len(c), frac)
    print(f"upfirdn {up}/{down}: worst err / bound {worst:.3f} (bound 1)")


def test_upfirdn_filter_shorter_than_up(rt):
    """A filter with fewer taps than `up` (3 taps, up = 5, down = 2, half_len = 1), which aware_upfirdn accepts: the output
    phases 3 and 4 meet no tap, contribute 0 and read nothing (before the fix `(nh - 1 - tap) / up` truncated toward zero and
    the loop read h[3], h[4]).  Reference: scipy.signal.upfirdn in float64 at rate 5 / 2; the kernel's
    y[j] = sum_i x[i] h[2 j - 5 i + 1] is scipy's output j + 1 for the filter delayed by one sample ([0, h0, h1, h2]),
    zero beyond scipy's end.  Same bound as above; an output without a tap has bound 0, so it must be exactly 0."""
    from scipy import signal
    up, down, half = 5, 2, 1
    rng = np.random.default_rng(102)
    h = np.array([0.75, -0.5, 0.3125], dtype=np.float32) + noise(rng, 3)
    clips = [noise(rng, 37), noise(rng, 8)]
    got = rt.upfirdn(rt.Ragged.from_list(clips), torch.from_numpy(h).cuda(), up, down, half).to_list()
    h64 = h.astype(np.float64)
    worst, untapped = 0.0, 0
    for c, y in zip(clips, got):
        n_out = -(-len(c) * up // down)
        assert y.shape == (n_out,)
        c64 = c.astype(np.float64)
        full = signal.upfirdn(np.concatenate([[0.0], h64]), c64, up, down)[1:]
        ref = np.zeros(n_out)
        ref[:min(n_out, len(full))] = full[:n_out]
        direct, bound = dot_terms(c64, h64, up, down, half, n_out)
        np.testing.assert_array_equal(ref, direct)                      # at most one product per output: no rounding to differ by
        assert np.all(full[n_out:] == 0.0)
        err = np.abs(y.astype(np.float64) - ref)
        assert np.all(err <= bound), np.max(err)
        no_tap = (np.arange(n_out) * down + half) % up >= len(h)        # phases 3 and 4: two outputs in five
        assert np.all(bound[no_tap] == 0) and not np.any(y[no_tap])
        untapped += int(no_tap.sum())
        worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))))
    assert untapped == 45
    print(f"upfirdn nh < up: worst err / bound {worst:.3f} (bound 1), {untapped} outputs without a tap are exactly 0")


# ---- 2. IIR ----------------------------------------------------------------------------------------------------------
IIR_KINDS = [(0.3, "low"), (0.5, "low"), (0.4, "highpass")]          # Butterworth cut-offs in units of Nyquist
LFILTER_LENS = [17, 2049, 1, 20001, 40, 4097, 16, 2048]              # chunk counts 2, 65, 1, 126, 3, 86, 1, 128
LFILTER_PADDED = 5                                                   # this clip's filter has order ncoef - 2, zero-padded
FILTFILT_PADDED = 4


def iir_filters(ncoef, count, padded_at):
    """One Butterworth filter of order ncoef - 1 per clip, cycling through IIR_KINDS; clip `padded_at` gets order ncoef - 2,
    zero-padded to ncoef coefficients.  Returns b, a [count, ncoef]."""
    from scipy import signal
    bs, as_ = [], []
    for i in range(count):
        wn, btype = IIR_KINDS[i % len(IIR_KINDS)]
        b, a = signal.butter(ncoef - 2 if i == padded_at else ncoef - 1, wn, btype)
        bs.append(np.concatenate([b, np.zeros(ncoef - len(b))]))
        as_.append(np.concatenate([a, np.zeros(ncoef - len(a))]))
    return np.stack(bs), np.stack(as_)


def filtfilt_lens(ncoef):
    return [3 * ncoef + 1, 4097, 3 * ncoef + 2, 20001, 100]         # scipy's minimum length is padlen + 1 = 3 ncoef + 1


@pytest.mark.parametrize("ncoef", range(2, 13))
def test_iir_lfilter_every_ncoef(rt, ncoef):
    """iir_kernel<ncoef>, mode 0, float64 out, a different filter per clip, against scipy.signal.lfilter in float64 to
    1e-12 * max(1, max|ref|), the bound of test_iir_time_parallel_long_ragged (for these filters the float64 recurrence
    and the same recurrence in 80-bit arithmetic differ by at most 1.4e-14 on these clips, ncoef 12 the worst: almost two
    orders of magnitude of margin).
    ncoef 10..12 take the second round of lanes in the matrix product, ncoef 2 is the one-state kernel.
    Measured on the MI355X: worst error 5.6e-17 (ncoef 2) rising to 1.4e-14 (ncoef 12)."""
    from scipy import signal
    rng = np.random.default_rng(200 + ncoef)
    clips = [noise(rng, n) for n in LFILTER_LENS]
    b, a = iir_filters(ncoef, len(clips), LFILTER_PADDED)
    y = rt.iir(rt.Ragged.from_list(clips), b, a, out_f64=True).to_list()
    worst = 0.0
    for i, c in enumerate(clips):
        ref = signal.lfilter(b[i], a[i], c.astype(np.float64))
        assert y[i].dtype == np.float64 and y[i].shape == ref.shape
        err = float(np.max(np.abs(y[i] - ref)))
        tol = 1e-12 * max(1.0, float(np.max(np.abs(ref))))
        worst = max(worst, err / tol)
        assert err < tol, (ncoef, len(c), err)
    print(f"lfilter ncoef {ncoef}: worst err / bound {worst:.2e} (bound 1e-12 * max(1, |ref|))")


@pytest.mark.parametrize("ncoef", range(2, 13))
def test_iir_filtfilt_every_ncoef(rt, ncoef):
    """iir_kernel<ncoef>, mode 1, float32 out, from scipy's minimum length 3 ncoef + 1 (the odd extension reads the clip's
    first and last sample without the clamps) to 20001 samples, lfilter_zi of each clip's own filter, against
    scipy.signal.filtfilt in float64 to 1.2e-7 * max(1, max|ref|) as test_iir_time_parallel_long_ragged.
    On the CPU scipy's float64 filtfilt and the same recurrence in 80-bit arithmetic agree to 5.8e-14 or better on every
    clip and filter of this test (worst: ncoef 12 at the minimum length), far below the 1e-9 the reference needs to be
    good to, so no cut-off had to move toward 0.5.
    Measured on the MI355X: equal to the rounded reference for ncoef 4..12; 1.5e-8 (ncoef 2), 7e-9 (ncoef 3)."""
    from scipy import signal
    rng = np.random.default_rng(300 + ncoef)
    clips = [noise(rng, n) for n in filtfilt_lens(ncoef)]
    b, a = iir_filters(ncoef, len(clips), FILTFILT_PADDED)
    zi = np.stack([signal.lfilter_zi(b[i], a[i]) for i in range(len(clips))])
    y = rt.iir(rt.Ragged.from_list(clips), b, a, zi, filtfilt=True).to_list()
    worst = 0.0
    for i, c in enumerate(clips):
        ref = signal.filtfilt(b[i], a[i], c.astype(np.float64))
        assert y[i].dtype == np.float32 and y[i].shape == ref.shape
        err = float(np.max(np.abs(y[i].astype(np.float64) - ref.astype(np.float32))))
        tol = 1.2e-7 * max(1.0, float(np.max(np.abs(ref))))
        worst = max(worst, err / tol)
        assert err <= tol, (ncoef, len(c), err)
    print(f"filtfilt ncoef {ncoef}: worst err / bound {worst:.3f} (bound 1.2e-7 * max(1, |ref|))")


def test_iir_refuses_an_empty_clip(rt):
    """A clip of length 0 has no chunk length (the kernel's nch = (cnt + L - 1) / L divided by zero): rt.iir refuses the
    batch before anything is launched, in both modes."""
    from scipy import signal
    b, a = signal.butter(4, 0.3)
    x = rt.Ragged(torch.zeros(100, dtype=torch.float32, device="cuda"), [60, 0, 40])
    with pytest.raises(ValueError, match="at least one sample"):
        rt.iir(x, np.tile(b, (3, 1)), np.tile(a, (3, 1)), out_f64=True)
    with pytest.raises(ValueError, match="at least one sample"):
        rt.iir(x, np.tile(b, (3, 1)), np.tile(a, (3, 1)), np.tile(signal.lfilter_zi(b, a), (3, 1)), filtfilt=True)


# ---- 3. Gaussian noise -----------------------------------------------------------------------------------------------
def test_gaussian_noise_ragged_tails(rt, O):
    """gaussian_noise_kernel writes four samples per Philox block behind `i < n`: lengths with every remainder mod 4, the
    shortest first, against the oracle per clip to one float32 rounding of the float64 sum, 2^-23 * max|ref|.  A silent clip
    has sigma = 0 and must come back bit for bit.
    Measured on the MI355X: every sample equal to the oracle's."""
    rng = np.random.default_rng(400)
    lens = [1, 2, 3, 5, 1023, 4097, 16001, 1022, 6]
    seeds = [0, 7, 2 ** 31 - 1, 12345, 1, 99991, 2 ** 16, 31, 2 ** 31 - 2]
    clips = [noise(rng, n) for n in lens]
    clips[7] = np.zeros(1022, dtype=np.float32)                         # silent
    out = rt.gaussian_noise(rt.Ragged.from_list(clips), 20.0, seeds).to_list()
    worst = 0.0
    for c, s, y in zip(clips, seeds, out):
        ref = O.gaussian_noise_attack(c, 20.0, s)
        assert y.shape == ref.shape and y.dtype == np.float32
        tol = 2.0 ** -23 * float(np.max(np.abs(ref)))
        err = float(np.max(np.abs(y.astype(np.float64) - ref.astype(np.float64))))
        assert err <= tol, (len(c), s, err, tol)
        worst = max(worst, err / tol if tol else 0.0)
        if len(c) > 100 and np.any(c):
            assert np.max(np.abs(y - c)) > 0                            # noise was added
    np.testing.assert_array_equal(out[7], clips[7])
    print(f"gaussian noise: worst err / bound {worst:.3f} (bound 2^-23 * max|ref|)")


# ---- 4. PCM and waveform normalisation -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def norm_clips():
    """The 1- and 5-sample clips sit between long ones; the maxima sit where a wrong partial count or segment would miss them."""
    rng = np.random.default_rng(500)
    lens = [4095, 1, 8193, 5, 20000, 4096, 4097]
    clips = [noise(rng, n) for n in lens]
    clips[2][8192] = 1.0                                                # peak exactly 1.0, alone in the third 4096-segment
    clips[4][9000] = -0.8125                                            # largest |x| negative, in the third 4096-segment
    clips[5][:] = 0.0                                                   # silent
    clips[6][4096] = 0.90625                                            # largest |x| is the last sample
    assert all(np.max(np.abs(c)) < 0.8 for i, c in enumerate(clips) if i not in (2, 4, 6))
    assert np.argmax(np.abs(clips[4])) == 9000 and np.argmax(np.abs(clips[6])) == 4096 and np.max(np.abs(clips[2])) == 1.0
    return clips


@pytest.mark.parametrize("bits", [8, 12, 16, 24])
def test_pcm_quantize_ragged(rt, O, norm_clips, bits):
    """pcm_quantize_kernel / absmax_into_scratch on a ragged batch (every clip is given the longest clip's partial count):
    integer work after one correctly rounded division, bit for bit against the oracle."""
    out = rt.pcm_quantize(rt.Ragged.from_list(norm_clips), bits).to_list()
    for c, y in zip(norm_clips, out):
        np.testing.assert_array_equal(y, O.pcm_bit_depth(c, bits))
    print(f"pcm {bits}: {len(norm_clips)} ragged clips bit-exact")


def test_waveform_normalize_ragged(rt, norm_clips):
    """normalize_kernel on the same batch: x / max(|x| + 1e-8) in float32, one correctly rounded division, bit for bit."""
    out = rt.waveform_normalize(rt.Ragged.from_list(norm_clips)).to_list()
    for c, y in zip(norm_clips, out):
        ref = c / np.max(np.abs(c) + np.float32(1e-8))
        assert ref.dtype == np.float32
        np.testing.assert_array_equal(y, ref)
    assert np.max(out[2]) == 1.0 and np.min(out[4]) == -1.0 and not np.any(out[5])
    print(f"waveform normalise: {len(norm_clips)} ragged clips bit-exact")


# ---- 5. segment cut and decimation -----------------------------------------------------------------------------------
def test_segment_cut_at_the_ends(A, rt, O):
    """segment_copy_kernel on a ragged batch with the cut at sample 0, ending at the clip's end and in the middle (each clip
    takes each in turn), through DeleteSamples / SampleSupression with given starts, and directly with a clip whose cut is
    empty.  Index work: bit for bit against the oracle."""
    rng = np.random.default_rng(600)
    lens = [1000, 4097, 161, 16000, 7]
    clips = [noise(rng, n) for n in lens]
    x = rt.Ragged.from_list(clips)
    p = 0.1
    cuts = [int(p * n) for n in lens]                                   # 100, 409, 16, 1600, 0
    for turn in range(3):
        starts = [[0, n - k, (n - k) // 2][(i + turn) % 3] for i, (n, k) in enumerate(zip(lens, cuts))]
        out = A.DeleteSamples(p).apply_batch(x, 16000, starts=starts).to_list()
        for c, s, y in zip(clips, starts, out):
            np.testing.assert_array_equal(y, O.delete_samples_attack(c, p, start=s))
    sr, ps = 16000, 0.01                                                # SampleSupression zeroes int(ps * sr) = 160 samples
    k = int(ps * sr)
    x4 = rt.Ragged.from_list(clips[:4])
    for turn in range(3):
        starts = [[0, n - k, (n - k) // 2][(i + turn) % 3] for i, n in enumerate(lens[:4])]
        out = A.SampleSupression(ps).apply_batch(x4, sr, starts=starts).to_list()
        for c, s, y in zip(clips[:4], starts, out):
            ref = O.sample_suppression_attack(c, ps, sr=sr, start=s)
            np.testing.assert_array_equal(y, ref)
            assert int((ref == 0).sum()) >= k
    # rt.segment_cut itself, a k = 0 clip between two others, both forms
    starts, ks = [0, 77, lens[2] - 16, 16000 - 5, 3], [100, 0, 16, 5, 0]
    for zero_fill in (False, True):
        out = rt.segment_cut(x, starts, ks, zero_fill=zero_fill).to_list()
        for c, s, kk, y in zip(clips, starts, ks, out):
            if zero_fill:
                ref = c.copy()
                ref[s:s + kk] = 0
            else:
                ref = np.concatenate([c[:s], c[s + kk:]])
            np.testing.assert_array_equal(y, ref)
    print("segment cut: delete / suppress at start 0, at the clip's end and in the middle, k = 0: bit-exact")


@pytest.mark.parametrize("sr,target", [(48000, 16000), (16000, 8000)], ids=["factor3", "factor2"])
def test_decimate_clips_shorter_than_the_factor(A, rt, O, sr, target):
    """decimate_interp_kernel on clips of 1 to 4 samples (shorter than, equal to and just past the factor) next to 1025:
    np.interp's float64 arithmetic, bit for bit against the oracle."""
    rng = np.random.default_rng(601)
    clips = [noise(rng, n) for n in (3, 1025, 1, 4, 2)]
    out = A.Resample(target).apply_batch(rt.Ragged.from_list(clips), sr).to_list()
    for c, y in zip(clips, out):
        assert y.dtype == np.float64
        np.testing.assert_array_equal(y, O.resample_attack(c, sr, target))
    print(f"decimate factor {sr // target}: clips of 3, 1025, 1, 4, 2 samples bit-exact")


# ---- 6. phase vocoder and spectral quantiser -------------------------------------------------------------------------
def shortest_clip_with_3_output_frames(rt, rate):
    t = 3
    while rt.phase_vocoder_frames([t], rate)[0] < 3:
        t += 1
    return max(513, 256 * (t - 1)), t                                   # 1 + n // 256 = t frames; reflect padding needs n > 512


@pytest.mark.parametrize("rate", [0.5, 1.0, 1.37, 2.0])
def test_time_stretch_at_the_frame_minimum(A, rt, O, rate):
    """phase_vocoder_kernel / rt.time_stretch on a ragged batch of 513 (3 frames), 769 (4 frames) and 9000 samples.  A clip
    that the rate would leave with fewer than 3 output frames is refused with the existing ValueError, asserted per clip,
    and replaced by the shortest clip that still leaves 3 (from rt.phase_vocoder_frames) plus the samples it had beyond 513.
    That happens at rate 2.0 only: len(arange(0, 3, 2)) = len(arange(0, 4, 2)) = 2, so 513 and 769 become 1024 and 1280
    samples (5 and 6 frames in, 3 out).  At 1.37 len(arange(0, 3, 1.37)) = 3: the 513-sample clip is taken as it stands,
    3 frames in and 3 out, as at rate 1.0; at 0.5 it gives 6.  Against the oracle with test_time_stretch_extension's bound,
    2e-5 * max(1, max|ref|).
    Measured on the MI355X: 0.091, 0.006, 0.017 and 0.026 of the bound at the four rates."""
    rng = np.random.default_rng(700)
    n_min, t_min = shortest_clip_with_3_output_frames(rt, rate)
    assert rt.phase_vocoder_frames([t_min], rate)[0] == 3 or rate < 1.0
    assert n_min == {0.5: 513, 1.0: 513, 1.37: 513, 2.0: 1024}[rate]
    long_clip = noise(rng, 9000)
    clips = []
    for n in (513, 769):
        c = noise(rng, n)
        if rt.phase_vocoder_frames([1 + n // 256], rate)[0] < 3:
            with pytest.raises(ValueError, match="shrink below 3 frames"):
                A.TimeStretch(rate).apply_batch(rt.Ragged.from_list([long_clip, c]), 16000)
            c = noise(rng, n_min + n - 513)
        clips.append(c)
    clips.append(long_clip)
    assert [len(c) for c in clips] == ([1024, 1280, 9000] if rate == 2.0 else [513, 769, 9000])
    y = A.TimeStretch(rate).apply_batch(rt.Ragged.from_list(clips), 16000).to_list()
    worst = 0.0
    for c, got in zip(clips, y):
        ref = O.time_stretch_attack(c, rate)
        assert got.shape == ref.shape, (got.shape, ref.shape)
        T = 1 + len(c) // 256
        assert len(got) == 256 * (len(np.arange(0, T, rate)) - 1)
        tol = 2e-5 * max(1.0, float(np.max(np.abs(ref))))
        err = float(np.max(np.abs(got - ref)))
        worst = max(worst, err / tol)
        assert err < tol, (len(c), err)
    assert len(y[0]) == (512 if rate >= 1.0 else 1280)                  # exactly 3 output frames where the rate shrinks
    print(f"time stretch rate {rate}: shortest clip {n_min}, worst err / bound {worst:.3f} (bound 2e-5 * max(1, |ref|))")


@pytest.fixture(scope="module")
def half_silent_clip():
    """16000 samples, the first 4096 exactly zero: frames 0..14 see only zeros (frame t covers samples 256 t - 512 ..
    256 t + 511, and the reflection of zeros is zeros), so output samples 0..3327 are built from silent frames alone."""
    c = noise(np.random.default_rng(800), 16000)
    c[:4096] = 0.0
    return c


SILENT_FRAMES, SILENT_SAMPLES = 15, 3328


def test_mp3_surrogate_on_silent_frames(A, O, half_silent_clip):
    """spectral_quantize_kernel on digitally silent frames: mx takes its 1e-12 floor, every magnitude is 0 and sc = 0, so
    those frames stay exactly 0 (the oracle puts 1e-12 there: below every bound).  The whole clip against the oracle with
    test_mp3_surrogate_extension's relative-L2 bound 2e-3.
    Measured on the MI355X: relative L2 1.8e-7."""
    out = A.MP3Surrogate(1.5, -60.0).apply(half_silent_clip, 16000)
    ref = O.mp3_surrogate_attack(half_silent_clip, 1.5, -60.0)
    assert out.shape == ref.shape == (15872,)
    assert np.all(np.isfinite(out))
    rel = float(np.linalg.norm(out - ref) / np.linalg.norm(ref))
    print(f"mp3 surrogate, silent head: relative L2 {rel:.2e} (bound 2e-3)")
    assert rel < 2e-3
    assert not np.any(out[:SILENT_SAMPLES])
    assert np.any(out[4096:])


@pytest.mark.parametrize("floor_db", [-60.0, -25.0])
def test_mp3_surrogate_backward_on_silent_frames(rt, O, half_silent_clip, floor_db):
    """spectral_quantize_bwd_kernel on the same clip against torch autograd on the oracle's mp3_surrogate_spectrum, with
    test_mp3_surrogate_is_differentiable's exclusion rule and cap (bad < 2e-4 * total).  On the silent frames the oracle's
    gradient is finite and exactly 0 on the CPU (torch's abs and angle have zero gradient at 0), so they are compared like
    the rest, and the device's gradient there must be exactly 0.
    Measured on the MI355X: 3.3e-7 of the largest gradient entry, no bin on the other side of a boundary, both floors."""
    from aware_amd.utils.audio import default_plan
    plan = default_plan()
    batch = rt.Batch([len(half_silent_clip)])
    spec = rt.stft(plan, batch, batch.pack([half_silent_clip]), normalize=False)      # [frames, 520] complex64
    assert not bool(spec[:SILENT_FRAMES, :513].abs().any()) and bool(spec[SILENT_FRAMES, :513].abs().any())
    g = torch.Generator().manual_seed(3)
    G = torch.complex(torch.randn(spec.shape, generator=g), torch.randn(spec.shape, generator=g)).cuda()
    x = spec.clone().requires_grad_(True)
    y = rt.SpectralQuantizeSTE.apply(x, 1.5, floor_db)
    (gx,) = torch.autograd.grad(y, x, grad_outputs=G)
    y, gx = y.detach().cpu(), gx.cpu()
    S = spec[:, :513].T.cpu().clone().requires_grad_(True)                             # [513, T]
    Y = O.mp3_surrogate_spectrum(S, 1.5, floor_db)
    (gS,) = torch.autograd.grad(Y, S, grad_outputs=G[:, :513].T.cpu())
    assert bool(torch.isfinite(gS).all()) and not bool(gS[:, :SILENT_FRAMES].abs().any())
    assert bool(torch.isfinite(gx).all())
    assert not bool(gx[:SILENT_FRAMES, :513].abs().any()) and not bool(y[:SILENT_FRAMES, :513].abs().any())
    same = (y[:, :513].T - Y.detach()).abs() <= 1e-5 * Y.detach().abs().max()
    bad, total = int((~same).sum()), same.numel()
    err = ((gx[:, :513].T - gS).abs() * same).max().item()
    print(f"mp3 surrogate backward, floor {floor_db}: err {err:.2e} (bound {2e-5 * gS.abs().max().item():.2e}), "
          f"bins on the other side of a quantiser boundary: {bad} of {total}")
    assert err < 2e-5 * gS.abs().max().item(), err
    assert bad < 2e-4 * total
