"""Attack-aware embedding (EXTENSION, parity unpinned: the reference optimises against the clean synthesis only).

A chain of up to four attacks applied to the normalised synthesis inside every iteration of the embed loop, so that the
optimiser sees what an attacker does to the signal.  This module parses / validates the chain and restates the model in torch:
`apply_chain` is the specification the device kernels (csrc/loop_attack_kernels.hip) are tested against and the CPU twin of
the loop's new stage.  For clip b (length Ny) at optimiser step s with seed_b:

    entry j:  r = philox4x32_10(counter (0, s, 1 + j, 1), key (seed_b, 0x5EED));  on = (r[0] + 0.5) / 2^32 < prob
      sample_suppression(seconds), k = int(seconds * sample_rate):  start = (r[1] * (Ny - k)) >> 32;  on: x[start:start+k] = 0
      gaussian_noise(snr_db):  sigma = sqrt(mean(x^2) / 10^(snr_db / 10)) of the current x, detached;  on: x += sigma * eps,
        eps_i from philox4x32_10((i // 4, s, 0, j), (seed_b, 0x5EED)), lanes paired through Box-Muller as the post-hoc
        GaussianNoise attack pairs them (at s = 0, j = 0 the two draw the same noise)

      reverberation(rt60 = lo or [lo, hi] seconds, drr_db), n_lo = int(lo * sample_rate), n_hi = int(hi * sample_rate):
        n_h = n_lo + ((r[2] * (n_hi - n_lo + 1)) >> 32) taps;  tail t_i = eps_i exp(-ln(1000) i / n_h), 1 <= i < n_h, eps the
        normals of normal_draws with the third counter word 8 (index 0 drawn and discarded);  direct path
        h_0 = 10^(drr_db / 20) sqrt(sum t_i^2);  on: x = (h * x)[0:Ny], h detached (the backward pass is the correlation with
        h).  At most one per chain; a noise entry behind it takes its sigma from the convolved signal.  At s = 0, j = 0 and a
        scalar rt60 this is the post-hoc attacks.Reverberation of the same seed.

      speed_change(cents = c or [lo, hi], -400 <= lo <= hi <= 400; a scalar c > 0 means [-c, c]),
        m_lo = ceil(65536 (2^(lo / 1200) - 1)), m_hi = floor(65536 (2^(hi / 1200) - 1)) in float64:
        m = m_lo + ((r[3] * (m_hi - m_lo + 1)) >> 32), R = 65536 + m: the clip played at R / 65536 of its speed.  The draw is
        uniform in that ratio, not in cents.  p_i = i R as a 64-bit integer in 16.16 fixed point, i0 = p_i >> 16,
        f = (p_i & 0xFFFF) / 65536 (exact in float32, so host and device agree on every index and fraction);
        on: x[i] = w_-1(f) x[i0 - 1] + w_0(f) x[i0] + w_1(f) x[i0 + 1] + w_2(f) x[i0 + 2], samples outside [0, Ny) read as
        zero, 0 where p_i > (Ny - 1) << 16; Catmull-Rom weights w_-1 = ((-f + 2) f - 1) f / 2, w_0 = ((3 f - 5) f^2 + 2) / 2,
        w_1 = ((-3 f + 4) f + 1) f / 2, w_2 = (f - 1) f^2 / 2.  The clip keeps its length (a faster one ends in zeros, a slower
        one is truncated); m = 0 is the identity; R is detached.  At most one per chain, and not beside a reverberation; a
        noise entry behind it takes its sigma from the resampled signal.

      time_stretch(rate = r or [lo, hi], 0.75 <= lo <= hi <= 4/3; a scalar r > 1 means [1 / r, r]; above 1 is faster and shorter),
        m_lo = ceil(65536 (lo - 1)), m_hi = floor(65536 (hi - 1)) in float64:
        m = m_lo + ((r[3] * (m_hi - m_lo + 1)) >> 32), Q = 65536 + m: the clip's duration divided by Q / 65536 at its own pitch,
        by plain overlap-add.  H = 256, N = 1024, w the periodic Hann window of N points in float32 (the loop's STFT window);
        a_t = (t H Q) >> 16 in 64-bit signed integers (arithmetic shift) for every integer t >= -2;
        on: x[n] = 1/2 sum_t w[n - t H + 512] x[n - t H + a_t] over the at most four t with 0 <= n - t H + 512 < N, samples
        outside [0, Ny) read as zero.  Every index is an integer, so host and device agree on every tap.  The clip keeps its
        length (a faster one ends in zeros, a slower one is truncated); m = 0 is the identity; Q is detached.  At most one per
        chain and not beside a reverberation; a speed_change may follow it directly (tempo and pitch then move independently,
        a pitch shift being the diagonal), and in no other place of such a chain.

      pitch_shift(cents = c or [lo, hi], parsed and drawn as speed_change's: m from r[3] on [m_lo, m_hi], R = 65536 + m),
        the coupled rate Q = ((1 << 32) + R // 2) // R in 64-bit integers (Q R is within R / 2 of 2^32), mq = Q - 65536,
        L_u = stretch_length(Ny, mq): on: x = speed_change(time_stretch(x, mq, L_u), m, Ny): the overlap-add stretches the clip
        to its true length L_u (about R / 65536 of Ny; zero outside [0, L_u)), and the resampling plays that at R / 65536 of its
        speed, so the pitch moves by the drawn interval and the duration stays: the one diagonal of the tempo-pitch plane that
        the pair above leaves most steps.  Linear in x; m = 0 is the identity; m is detached.  At most one per chain, and not in
        a chain with a reverberation, a speed change or a time stretch.

      phase_vocoder(rate = r or [lo, hi], cents = c or [lo, hi]; at least one of the two; rate parsed and refused exactly as
        time_stretch's, cents exactly as speed_change's): with both keys the mode is stretch where r[2] < 2^31, else pitch; with
        one key it is that key's mode.  Stretch mode: mq = stretch_offset(r[3], *stretch_range), m = 0.  Pitch mode:
        m = speed_offset(r[3], *speed_range), mq = pitch_offsets(m)[1] - 65536 (the coupled rate of pitch_shift, inside the
        stretch's range for +-400 cents).  Q = 65536 + mq.  on: x = speed_change(pv_stretch(x, mq), m), both Ny long.
        pv_stretch(x, mq): S = STFT(x) on the loop's geometry (reflect-centred, periodic Hann 1024, hop 256, T = Ny / 256 + 1
        frames); for t = 0 .. T - 1: p = t Q in int64, i = p >> 16, al = (p & 0xFFFF) / 65536 (exact in float32, so host and
        device agree on every index and weight); Y[t] = 0 where i >= T, otherwise Y[t] = ((1 - al) |S[i]| + al |S[i + 1]|) P[t]
        with S[T] := 0; P[0] = u(S[0]), P[t + 1] = P[t] u(S[i + 1]) conj(u(S[i])); u(c) = c / |c|, and u(c) = 1 for a zero cell:
        one whose real and imaginary parts both compare equal to 0; x' = iSTFT(Y), the loop's iSTFT: T frames give Ny samples.
        mq = 0 and m = 0 returns x; a faster clip ends in zeros, a slower one is truncated.  P is the textbook accumulator in
        product form: acc += adv + princarg(dtheta - adv) is acc += dtheta modulo 2 pi when the two hops are equal, so it is the
        phase of oracle.phase_vocoder without an atan2 and without sensitivity to where the wrap falls.  P, Q and m are
        detached (no phase gradients) and d|c|/dc is torch's, 0 at 0, so the backward pass of pv_stretch is: the iSTFT adjoint,
        gm[t] = Re(conj(P[t]) G[t]), the transpose of the two-tap interpolation onto the input frames over ascending t,
        gS[i] = gmag[i] u(S[i]) (0 at a zero cell), the STFT adjoint.  At most one per chain, and not in a chain with a
        reverberation, a speed change, a time stretch or a pitch shift, in either order; element-wise entries may stand in front
        of it and behind it, and a noise entry behind it takes its sigma from the vocoded signal.

      delete_samples(seconds = v or [lo, hi], at = "start" or "anywhere"): a scalar v means k_lo = 1, k_hi = int(v * sample_rate);
        a pair k_lo = int(lo * sample_rate), k_hi = int(hi * sample_rate); 1 <= k_lo <= k_hi < Ny.
        k = k_lo + ((r[2] * (k_hi - k_lo + 1)) >> 32);  start = 0 for at: start (the reference's Cropout), otherwise
        suppression_start(r[1], Ny, k) = (r[1] * (Ny - k)) >> 32 (its DeleteSamples);
        on: z[i] = x[i] for i < start, x[i + k] for start <= i < Ny - k, 0 for i >= Ny - k: k samples are cut out, the remainder
        moves up and the clip keeps its length, as under the speed and stretch kinds.  Every index is an integer and every
        value a copy, so host and device agree bit for bit.  The backward pass is the exact adjoint in gather form:
        gx[i] = gz[i] for i < start, 0 for start <= i < start + k, gz[i - k] for i >= start + k.  At most one per chain, and not
        in a chain with a reverberation, a speed change, a time stretch, a pitch shift or a phase vocoder, in either order;
        element-wise entries may stand in front of it and behind it, and a noise entry behind it takes its sigma from the
        shortened signal.

      gain_envelope(period = v or [lo, hi] seconds, floor = 0.0), P_lo = int(lo * sample_rate), P_hi = int(hi * sample_rate),
        64 <= P_lo <= P_hi <= 2^20, 0 <= floor < 1: a gain that moves over time (a fade, ducking, tremolo, an AGC riding the level):
        P = P_lo + ((r[2] * (P_hi - P_lo + 1)) >> 32) samples between breakpoints, ph = (r[1] * P) >> 32 the phase of the first;
        breakpoint k >= 0: w_k = philox4x32_10((k // 4, s, 16 + j, 0), (seed_b, 0x5EED))[k % 4] (the third counter words 16..19
        are the envelopes': 0 is noise, 1..4 the entry draws, 8 the responses, 12 the mixture), u_k = (w_k >> 8) 2^-24 (exact in
        float32), g_k = floor + (1 - floor) u_k in float32, so floor <= g_k <= 1;  at sample i: pos = i + ph, k = pos // P,
        f = float32(pos - k P) / float32(P), g(i) = g_k + f (g_{k+1} - g_k): piecewise linear, continuous;  on: x[i] *= g(i).
        A period longer than the clip is valid: the clip then sees one ramp.  g is detached: the backward pass is gx[i] = g(i) gz[i],
        the same operator.  Element-wise as noise and suppression are: it does not split a chain, any number of entries may
        stand in front of or behind a splitting entry and in every chain of a mixture, and a noise entry behind it takes its
        sigma from the enveloped signal.  Host and device agree on g to 1e-6 (the division and the fused multiply-add).

      band_filter(response = "lowpass" | "highpass" | "bandpass" | "bandstop" or a list of them, freq = f or [lo, hi] in Hz,
        min_width = 400.0 Hz): a frequency-selective channel (a telephone line, a small speaker, a notch), a zero-phase
        windowed-sinc FIR of 255 taps.  Frequencies travel as integers c = round(65536 f / sample_rate), in units of 1 / 65536
        cycle per sample (Nyquist is 32768): c_lo, c_hi, w_min (filter_range).  mask = the sum of the responses' bits
        (lowpass 1, highpass 2, bandpass 4, bandstop 8);  e1 = c_lo + ((r[1] * (c_hi - c_lo + 1)) >> 32), e2 the same from r[2];
        response = the ((r[3] * popcount(mask)) >> 32)-th set bit of mask, counted from the lowest;  lowpass and highpass:
        c1 = e1;  band responses: c1 = min(e1, e2), c2 = max(e1, e2), and c2 = c1 + w_min if c2 - c1 < w_min (filter_draw).
        Taps, k = -127..127 (filter_taps): w[k] = 0.54 + 0.46 cos(pi k / 127), lp_c[0] = c / 32768,
        lp_c[k] = w[k] sin(2 pi ((c |k|) mod 65536) / 65536) / (pi |k|) (the phase reduced in integers), delta the unit impulse;
        h = lp_c1, delta - lp_c1, lp_c2 - lp_c1, delta - (lp_c2 - lp_c1).  on: z[i] = sum_k h[k] x[i - k], x zero outside the
        clip (band_filter): the clip keeps its length and there is no delay.  h is symmetric and the extension is by zeros, so
        the operator is its own adjoint.  At most one per chain, and not in a chain with any other splitting kind, in either
        order; element-wise entries may stand in front of it (noise there is coloured noise) and behind it (noise there takes
        its sigma from the filtered signal).  Host and device agree on h to 1e-6.

      excerpt(seconds = v or [lo, hi]), L_lo = int(lo * sample_rate), L_hi = int(hi * sample_rate), 1024 <= L_lo <= L_hi (a
        scalar is a fixed length): what a detector sees of an excerpt of the clip.
        L = min(L_lo + ((r[2] * (L_hi - L_lo + 1)) >> 32), Ny), and L = Ny where the entry does not fire;
        start = (r[1] * (Ny - L + 1)) >> 32, so 0 <= start <= Ny - L (excerpt_draw);
        z[i] = x[start + (i mod L)] (excerpt_tile): the excerpt repeated periodically until it fills the clip, which keeps its
        length.  The model card's convolutions are 1 x 1, so time couples only through the norms' statistics and the read-out's
        mean, and the periodic repetition has both as the excerpt alone has them, up to the frames at the seams; zeros
        outside the excerpt would enter those statistics.  Every value is a copy, so host and device agree bit for bit.  The
        backward pass is the exact adjoint in gather form (excerpt_tile_adjoint): gx[i] = sum_m gz[(i - start) + m L] for
        start <= i < start + L over m = 0, 1, .. while the index is below Ny, 0 outside; in float32 the sum runs over
        ascending m, the first term copied and every further one a single rounded addition, so host and device agree bit for
        bit there too.  L = Ny is the identity in both directions: a clip shorter than L_lo is left alone, not refused.  At
        most one per chain, and not in a chain with any other splitting kind, in either order; element-wise entries may stand
        in front of it and behind it, and a noise entry behind it takes its sigma from the tiled signal.

      time_warp(depth = d, period = v or [lo, hi]), 0 < d <= 0.1, D = floor(65536 d) in float64, so 1 <= D <= 6553; period in
        seconds, default [0.032, 0.512]: the clip resampled at a rate that is piecewise linear in time between drawn
        breakpoints: wow and flutter, a drifting sample clock, a deliberate desynchronisation.  The breakpoints are a power of two
        apart, so that nothing divides: e_lo = ceil(log2(int(lo * sample_rate))), e_hi = floor(log2(int(hi * sample_rate))),
        8 <= e_lo <= e_hi <= 20; a scalar v means e_lo = e_hi = round(log2(int(v * sample_rate))) (warp_range).
        e = e_lo + ((r[2] * (e_hi - e_lo + 1)) >> 32), P = 2^e, ph = (r[1] * P) >> 32 (warp_draw).  For breakpoint k >= 0:
        w_k = philox4x32_10((k // 4, s, 20 + j, 0), (seed_b, 0x5EED))[k % 4] (the third counter words 20..23 are this kind's; 0,
        1..4, 8, 12 and 16..19 are taken), m_k = -D + ((w_k * (2 D + 1)) >> 32), R_k = 65536 + m_k (warp_rates).
        In signed 64-bit integers, >> arithmetic (warp_positions): A(0) = 0, A(k + 1) = A(k) + P R_k + (((R_{k+1} - R_k) P) >> 1);
        for u >= 0 with k = u >> e and t = u & (P - 1), Pos(u) = A(k) + t R_k + (((R_{k+1} - R_k) t t) >> (e + 1)): continuous at
        the breakpoints by construction, strictly increasing because every rate is at least 0.9; p_i = Pos(i + ph) - Pos(ph).
        i0 = p_i >> 16, f = (p_i & 0xFFFF) / 65536, and z[i] is the speed change's Catmull-Rom tap at (i0, f), samples outside
        [0, Ny) read as zero, z[i] = 0 where p_i > (Ny - 1) << 16 (time_warp): the clip keeps its length.  An entry that does not
        fire copies the clip.  The rates are detached.  The backward pass is the exact adjoint in gather form
        (time_warp_adjoint): gx[j] = sum over ascending i of w_{j - i0(i)}(f_i) gz[i].  At most one per chain, and not in a chain
        with any other splitting kind, in either order; element-wise entries may stand in front of it and behind it, and a noise
        entry behind it takes its sigma from the warped signal.  At a depth of 0.01 or less the plain watermark already reads
        0 %: the kind buys robustness against strong warps.

      frequency_shift(hz = v or [lo, hi]; a scalar v > 0 means [-v, v]): single-sideband modulation, every component of the clip
        moved by the same number of Hz: a mistuned SSB or heterodyne link, an analogue carrier system, a deliberate
        desynchronisation.  Neither a pitch shift nor a speed change: those scale frequencies.  Shifts travel as signed integers
        d = round(hz / sample_rate 2^20), in units of sample_rate / 2^20 Hz, |d| <= 65536 (sample_rate / 16): d_lo, d_hi
        (shift_range).  Phases are integers in units of 2^-20 turn.  d = d_lo + ((r[1] * (d_hi - d_lo + 1)) >> 32),
        p0 = r[2] >> 12, r[3] unused (shift_draw).  Hilbert taps, k = -127..127 (hilbert_taps): w[k] = 0.54 + 0.46 cos(pi k / 127),
        h[k] = w[k] 2 / (pi k) for odd k, 0 for even k, zero included; h is antisymmetric and sum|h| = 3.4103.
        (Hx)[i] = sum_k h[k] x[i - k], x zero outside the clip;  theta_i = (p0 + i d) mod 2^20, phi_i = 2 pi theta_i / 2^20;
        on: z[i] = x[i] cos phi_i - (Hx)[i] sin phi_i (frequency_shift): a positive d shifts upwards, the clip keeps its length
        and there is no delay.  d and p0 are detached.  The backward pass is the exact adjoint (frequency_shift_adjoint):
        gx[j] = g[j] cos phi_j + (H(g sin phi))[j], because H^T = -H under the extension by zeros.  On a signal band-limited to
        150-7000 Hz at 16 kHz the operator equals the FFT analytic-signal shift to a relative L2 of 4.1e-4 over the interior of
        a 1 s clip; below about 150 Hz the 255-tap transformer leaves some of the image sideband: a property of the model.  At
        most one per chain, and not in a chain with any other splitting kind, in either order; element-wise entries may stand in
        front of it and behind it, and a noise entry behind it takes its sigma from the shifted signal.  The kind buys the
        range it draws and nothing outside it, and it does not help against the phase vocoder's pitch shift (DESIGN.md
        section 37).

In the loop x = N(N(y)) of the raw synthesis y, N(v) = v / (max|v| + 1e-8), and the analysis (N, N, STFT, band magnitudes)
runs on the chain's output."""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np
import torch

MAX_ATTACKS = 4
_KEY1 = 0x5EED
MAX_IR = 8192                   # taps of the longest impulse response
_IR_WORD = 8                    # third Philox counter word of the impulse responses (0: noise, 1..4: entry draws)
MAX_CENTS = 400.0               # widest speed change or pitch shift either way
MIN_RATE, MAX_RATE = 0.75, 4.0 / 3.0            # slowest and fastest time stretch
STRETCH_HOP, STRETCH_WIN = 256, 1024            # the overlap-add's hop and window: the loop's STFT geometry
DELETE_AT = {"start": 0, "anywhere": 1}         # where a sample deletion cuts: param[2] of the C ABI's entry
MIN_PERIOD, MAX_PERIOD = 64, 1 << 20            # samples between two breakpoints of a gain envelope
_ENV_WORD = 16                  # third Philox counter word of entry j's breakpoints is 16 + j
RESPONSES = {"lowpass": 1, "highpass": 2, "bandpass": 4, "bandstop": 8}      # the bits of a band filter's mask: param[0]
FILTER_HALF = 127               # taps on either side of a band filter's centre
MAX_EDGE = 32767                # the highest edge, in units of 1 / 65536 cycle per sample: one below Nyquist
MIN_EXCERPT = 1024              # samples of the shortest excerpt a chain may draw
MIN_WARP_EXP, MAX_WARP_EXP = 8, 20              # a time warp's breakpoints are 2^e samples apart
MAX_WARP_DEPTH = 6553           # the widest rate offset D of a time warp: a tenth either way, floor(65536 * 0.1)
WARP_PERIOD = [0.032, 0.512]    # a time warp's default period in seconds
_WARP_WORD = 20                 # third Philox counter word of entry j's rates is 20 + j
PHASE_ONE = 1 << 20             # a frequency shift's phases are integers in units of 1 / PHASE_ONE turn
MAX_SHIFT = 65536               # the widest frequency shift either way, in units of sample_rate / PHASE_ONE Hz: sample_rate / 16


def kind_id(kind) -> int | None:
    """The C ABI's number of a chain kind (AWARE_LOOP_* of include/aware_hip.h), None for an unknown one."""
    return KINDS.get(kind) if isinstance(kind, str) else None


# The one-split rule (csrc/loop_chain.hpp holds the device's statement of it): the kinds of SPLITTING and of STAGED need launches
# of their own between two stages of element-wise entries, and a chain holds at most one entry of them.  The one exception is
# the pair: a speed change directly behind a time stretch.
def _one_split(j: int, kind: str, out: list[dict]) -> None:
    """ValueError if entry j of a splitting kind may not join the entries `out` in front of it.  The message names the kind
    itself if the chain holds it already, otherwise the last splitting entry, the later of the two in SPLITTING + STAGED first."""
    order = SPLITTING + STAGED
    held = [o["kind"] for o in out if o["kind"] in order]
    if not held or (kind == "speed_change" and held == ["time_stretch"] and out[-1]["kind"] == "time_stretch"):
        return
    head = f"loop_attacks[{j}] ({kind}): "
    if kind in held:
        raise ValueError(head + f"at most one {_KIND[kind].display} per chain")
    if {kind, held[-1]} == {"speed_change", "time_stretch"}:
        raise ValueError(head + ("beside a time stretch, the speed change follows it directly" if kind == "speed_change"
                                 else "a speed change in the same chain follows the stretch directly"))
    first, second = sorted((kind, held[-1]), key=order.index, reverse=True)
    raise ValueError(head + f"a chain holds a {_KIND[first].display} or a {_KIND[second].display}, not both")


def _number_or_pair(head: str, a: dict, key: str, scalar: str = "same", ok=lambda lo, hi: 0.0 < lo <= hi, needs: str = "0 < lo <= hi",
                    catch=(TypeError, ValueError), default=None):
    """The parameter a[key], a number or [lo, hi], as it goes into the parsed entry: [lo, hi] in floats.  `scalar` says what a
    number v means: "same" [v, v]; "keep" the same range, and the number itself is returned; "neg" [-v, v], for v > 0 only;
    "inv" [1 / v, v], for v > 1 only.  ValueError with `head` in front: a missing key without a `default`, what is neither a
    number nor a list of two (the exceptions of `catch`; a ValueError of float() passes where it is not among them), a scalar
    outside its rule, values that are not finite or not ok(lo, hi), which the message states as `needs`."""
    if key not in a and default is None:
        raise ValueError(head + f"{key} is required")
    v = a.get(key, default)
    pair = isinstance(v, (list, tuple))
    try:
        if pair and len(v) != 2:
            raise TypeError
        lo, hi = (float(v[0]), float(v[1])) if pair else (float(v), float(v))
    except catch:
        raise ValueError(head + f"{key} = {v!r} is neither a number nor [lo, hi]") from None
    if not pair and scalar in ("neg", "inv"):
        least = 0.0 if scalar == "neg" else 1.0
        if not hi > least:
            raise ValueError(head + f"a scalar {key} has to be > {least:g}; got {v!r}")
        lo = -hi if scalar == "neg" else 1.0 / hi
    if not (math.isfinite(lo) and math.isfinite(hi) and ok(lo, hi)):
        raise ValueError(head + f"{key} needs {needs}, both finite; got {v!r}")
    return hi if scalar == "keep" and not pair else [lo, hi]


def _parse_rate(head: str, a: dict) -> list[float]:
    """[lo, hi] of a time_stretch or phase_vocoder entry's rate: a scalar r > 1 means [1 / r, r]; 0.75 <= lo <= hi <= 4/3, and
    at least one offset inside."""
    rate = _number_or_pair(head, a, "rate", "inv", lambda lo, hi: MIN_RATE <= lo <= hi <= MAX_RATE, f"{MIN_RATE:g} <= lo <= hi <= 4/3",
                           catch=(TypeError,))
    m_lo, m_hi = stretch_range({"rate": rate})
    if m_lo > m_hi:
        raise ValueError(head + f"rate = {a['rate']!r} holds no offset (m_lo = {m_lo} > m_hi = {m_hi}, in units of 1 / 65536)")
    return rate


def _parse_cents(head: str, a: dict) -> list[float]:
    """[lo, hi] of a speed_change, pitch_shift or phase_vocoder entry's cents: a scalar c > 0 means [-c, c];
    -400 <= lo <= hi <= 400, and at least one speed offset inside."""
    cents = _number_or_pair(head, a, "cents", "neg", lambda lo, hi: -MAX_CENTS <= lo <= hi <= MAX_CENTS,
                            f"-{MAX_CENTS:g} <= lo <= hi <= {MAX_CENTS:g}", catch=(TypeError,))
    m_lo, m_hi = speed_range({"cents": cents})
    if m_lo > m_hi:
        raise ValueError(head + f"cents = {a['cents']!r} holds no speed offset (m_lo = {m_lo} > m_hi = {m_hi}, in units of 1 / 65536)")
    return cents


def _parse_filter(head: str, a: dict, sample_rate: int) -> dict:
    """response (a list of names, in the order of their bits), freq [lo, hi] and min_width of a band_filter entry."""
    if "response" not in a:
        raise ValueError(head + "response is required")
    if "freq" not in a:
        raise ValueError(head + "freq is required")
    rs = a["response"]
    names = [rs] if isinstance(rs, str) else list(rs) if isinstance(rs, (list, tuple)) else None
    if not names or any(not isinstance(r, str) or r not in RESPONSES for r in names):
        raise ValueError(head + f"response = {rs!r}; available: {list(RESPONSES)}, one or a list of them")
    fq = a["freq"]
    try:
        if isinstance(fq, (list, tuple)):
            if len(fq) != 2:
                raise TypeError
            lo, hi = float(fq[0]), float(fq[1])
        else:
            lo = hi = float(fq)
        mw = float(a.get("min_width", 400.0))
    except (TypeError, ValueError):
        raise ValueError(head + f"freq = {fq!r} is neither a number nor [lo, hi], or min_width = {a.get('min_width')!r} is "
                         f"not a number") from None
    if not (math.isfinite(lo) and math.isfinite(hi) and math.isfinite(mw)):
        raise ValueError(head + f"freq and min_width have to be finite; got {fq!r}, {a.get('min_width', 400.0)!r}")
    if not mw > 0.0:
        raise ValueError(head + f"min_width = {mw} has to be > 0")
    if lo > hi:
        raise ValueError(head + f"freq needs lo <= hi; got {fq!r}")
    e = {"response": [r for r in RESPONSES if r in names], "freq": [lo, hi], "min_width": mw}
    c_lo, c_hi, w_min = filter_range(e, sample_rate)
    if not (lo > 0.0 and hi < 0.5 * sample_rate - mw and 1 <= c_lo <= c_hi and w_min >= 1 and c_hi + w_min <= MAX_EDGE):
        raise ValueError(head + f"freq = {fq!r} Hz has an edge outside (0, Nyquist - min_width) = (0, "
                         f"{0.5 * sample_rate - mw:g}) at {sample_rate} Hz")
    return e


def _number(head: str, a: dict, key: str, ok, needs: str, default=None) -> float:
    """The parameter a[key] as a float.  ValueError with `head` in front: a missing key without a `default`, what is no number,
    a value that is not finite or not ok(v), which the message states as `needs`."""
    if key not in a and default is None:
        raise ValueError(head + f"{key} is required")
    try:
        v = float(a.get(key, default))
    except (TypeError, ValueError):
        raise ValueError(head + f"{key} = {a.get(key)!r} is not a number") from None
    if not (math.isfinite(v) and ok(v)):
        raise ValueError(head + f"{key} needs {needs}, finite; got {a.get(key)!r}")
    return v


def _in_range(head: str, range_of, e: dict, sample_rate: int) -> dict:
    """The parameters e if range_of(e, sample_rate), one of the *_range helpers, takes them; its ValueError behind `head` if not."""
    try:
        range_of(e, sample_rate)
    except ValueError as err:
        raise ValueError(head + f"{err}") from None
    return e


# One parser per kind, parse(head, a, sample_rate): the parameters of the entry a as the parsed entry holds them, behind kind and prob.
def _parse_noise(head, a, sample_rate):
    if "snr_db" not in a or not math.isfinite(float(a["snr_db"])):
        raise ValueError(head + "a finite snr_db is required")
    return {"snr_db": float(a["snr_db"])}


def _parse_suppression(head, a, sample_rate):
    if "seconds" not in a or not math.isfinite(float(a["seconds"])) or float(a["seconds"]) <= 0.0:
        raise ValueError(head + "seconds > 0 is required")
    return {"seconds": float(a["seconds"])}


def _parse_reverberation(head, a, sample_rate):
    e = {"rt60": _number_or_pair(head, a, "rt60"), "drr_db": float(a.get("drr_db", -3.0))}
    if not math.isfinite(e["drr_db"]):
        raise ValueError(head + "a finite drr_db is required")
    return e


def _parse_vocoder(head, a, sample_rate):
    if "rate" not in a and "cents" not in a:
        raise ValueError(head + "at least one of rate and cents is required")
    return {key: parse(head, a) for key, parse in (("rate", _parse_rate), ("cents", _parse_cents)) if key in a}


def _parse_delete(head, a, sample_rate):
    e = {"seconds": _number_or_pair(head, a, "seconds", "keep"), "at": a.get("at", "start")}
    if not isinstance(e["at"], str) or e["at"] not in DELETE_AT:
        raise ValueError(head + f"at = {e['at']!r}; available: {list(DELETE_AT)}")
    return e


def _parse_envelope(head, a, sample_rate):
    e = {"period": _number_or_pair(head, a, "period"),
         "floor": _number(head, a, "floor", lambda v: 0.0 <= v < 1.0, "0 <= floor < 1", default=0.0)}
    return _in_range(head, envelope_range, e, sample_rate)


def _parse_warp(head, a, sample_rate):
    depth = _number(head, a, "depth", lambda v: 0.0 < v <= 0.1, "0 < depth <= 0.1")
    return _in_range(head, warp_range, {"period": _number_or_pair(head, a, "period", "keep", default=WARP_PERIOD), "depth": depth}, sample_rate)


def _parse_shift(head, a, sample_rate):
    hz = _number_or_pair(head, a, "hz", "neg", lambda lo, hi: lo <= hi, "lo <= hi")
    return _in_range(head, shift_range, {"hz": hz}, sample_rate)


def parse_chain(chain, sample_rate: int = 16000) -> list[dict]:
    """Validated copy of a chain such as [{"kind": "gaussian_noise", "snr_db": 10.0, "prob": 1.0},
    {"kind": "sample_suppression", "seconds": 0.3, "prob": 0.75}] (None / empty: no chain).  ValueError: unknown kind or key,
    a missing parameter, prob outside [0, 1], a non-finite snr_db, seconds <= 0, more than four entries, a second entry of the
    SPLITTING kinds other than a speed change directly behind a time stretch (_one_split); and per kind, for
    {"kind": "reverberation", "rt60": 0.3 | [0.1, 0.5], "drr_db": -3.0}: a missing rt60, rt60 not 0 < lo <= hi (finite), a
    non-finite drr_db; for {"kind": "speed_change", "cents": 200.0 | [-50.0, 120.0]} and {"kind": "pitch_shift", "cents": ...}:
    a missing cents, a scalar <= 0, cents not -400 <= lo <= hi <= 400 (finite), a range that holds no speed offset
    (m_lo > m_hi); for {"kind": "time_stretch", "rate": 1.1 | [0.9, 1.1]}: a missing rate, a scalar <= 1, rate not
    0.75 <= lo <= hi <= 4/3 (finite), a range that holds no offset; for {"kind": "phase_vocoder", "rate": 1.15 | [0.85, 1.15],
    "cents": 150.0 | [-50.0, 120.0]}: neither key, what a time stretch's rate or a speed change's cents are refused for; for
    {"kind": "delete_samples", "seconds": 0.032 | [0.01, 0.2], "at": "start" | "anywhere"}: a missing seconds, seconds not
    0 < lo <= hi (finite), more or fewer than two values in a list, an unknown at; for {"kind": "gain_envelope",
    "period": 0.25 | [0.05, 0.5], "floor": 0.0}: a missing period, period not 0 < lo <= hi (finite), a period that is not
    64 <= P_lo <= P_hi <= 2^20 samples at `sample_rate`, floor not 0 <= floor < 1 (finite); for {"kind": "band_filter",
    "response": "lowpass" | ["lowpass", "bandstop"], "freq": 1000.0 | [600.0, 3800.0], "min_width": 400.0}: a missing freq or
    response, an unknown response, a non-finite value, lo > hi, an edge outside (0, Nyquist - min_width) at `sample_rate`,
    min_width <= 0; for {"kind": "excerpt", "seconds": 0.5 | [0.1875, 0.625]}: a missing seconds, seconds not 0 < lo <= hi
    (finite), more or fewer than two values in a list, fewer than 1024 samples at `sample_rate`; for
    {"kind": "time_warp", "depth": 0.04, "period": 0.128 | [0.032, 0.512]}: a missing depth, depth not 0 < depth <= 0.1 (finite)
    or below 1 / 65536, period not 0 < lo <= hi (finite), more or fewer than two values in a list, a period that holds no power
    of two from 2^8 to 2^20 samples at `sample_rate`; for {"kind": "frequency_shift", "hz": 120.0 | [-50.0, 120.0]}: a missing
    hz, a scalar <= 0, hz not lo <= hi (finite), more or fewer than two values in a list, a shift beyond sample_rate / 16
    either way (the periods, these edges and shifts and the excerpt's least length are the rules that read `sample_rate`).
    The unknown-kind message names the twelve kinds up to time_warp, as it always has; the table below is complete."""
    if not chain:
        return []
    if isinstance(chain, dict) or not isinstance(chain, (list, tuple)):
        raise ValueError("loop_attacks: a list of {kind: ...} entries is expected")
    if len(chain) > MAX_ATTACKS:
        raise ValueError(f"loop_attacks: at most {MAX_ATTACKS} entries, got {len(chain)}")
    out = []
    for j, a in enumerate(chain):
        if not isinstance(a, dict) or kind_id(a.get("kind")) is None:
            raise ValueError(f"loop_attacks[{j}]: unknown kind {a.get('kind') if isinstance(a, dict) else a!r}; available: {list(KINDS)[:_NAMED]}")
        k = _KIND[a["kind"]]
        head = f"loop_attacks[{j}] ({k.name}): "
        if set(a) - k.keys:
            raise ValueError(head + f"unknown key(s) {sorted(set(a) - k.keys)}")
        e = {"kind": k.name, "prob": float(a.get("prob", 1.0))}
        if not 0.0 <= e["prob"] <= 1.0:
            raise ValueError(head + f"prob = {e['prob']} outside [0, 1]")
        if k.splits or k.name in STAGED:
            _one_split(j, k.name, out)
        out.append({**e, **k.parse(head, a, sample_rate)})
    return out


def suppression_samples(entry: dict, sample_rate: int) -> int:
    """k = int(seconds * sample_rate), as SampleSupression.apply counts them."""
    return int(entry["seconds"] * sample_rate)


def reverb_taps(entry: dict, sample_rate: int) -> tuple[int, int]:
    """(n_lo, n_hi) = (int(lo * sample_rate), int(hi * sample_rate)) of a parsed reverberation entry."""
    return int(entry["rt60"][0] * sample_rate), int(entry["rt60"][1] * sample_rate)


def speed_range(entry: dict) -> tuple[int, int]:
    """(m_lo, m_hi) = (ceil(65536 (2^(lo / 1200) - 1)), floor(65536 (2^(hi / 1200) - 1))) of a parsed speed_change or pitch_shift entry, in
    float64: the speed offsets, in units of 1 / 65536, that lie inside the range of cents."""
    lo, hi = entry["cents"]
    return (int(math.ceil(65536.0 * (2.0 ** (lo / 1200.0) - 1.0))), int(math.floor(65536.0 * (2.0 ** (hi / 1200.0) - 1.0))))


def stretch_range(entry: dict) -> tuple[int, int]:
    """(m_lo, m_hi) = (ceil(65536 (lo - 1)), floor(65536 (hi - 1))) of a parsed time_stretch entry, in float64: the offsets of
    the rate from 1, in units of 1 / 65536, that lie inside the range."""
    lo, hi = entry["rate"]
    return int(math.ceil(65536.0 * (lo - 1.0))), int(math.floor(65536.0 * (hi - 1.0)))


def delete_range(entry: dict, sample_rate: int) -> tuple[int, int]:
    """(k_lo, k_hi) of a parsed delete_samples entry: (1, int(v * sample_rate)) for a scalar v, (int(lo * sample_rate),
    int(hi * sample_rate)) for a pair."""
    sec = entry["seconds"]
    if isinstance(sec, (list, tuple)):
        return int(sec[0] * sample_rate), int(sec[1] * sample_rate)
    return 1, int(sec * sample_rate)


def envelope_range(entry: dict, sample_rate: int) -> tuple[int, int]:
    """(P_lo, P_hi) = (int(lo * sample_rate), int(hi * sample_rate)) of a parsed gain_envelope entry: samples between two
    breakpoints.  ValueError unless 64 <= P_lo <= P_hi <= 2^20."""
    p_lo, p_hi = int(entry["period"][0] * sample_rate), int(entry["period"][1] * sample_rate)
    if not MIN_PERIOD <= p_lo <= p_hi <= MAX_PERIOD:
        raise ValueError(f"period = {entry['period']} s is {p_lo}..{p_hi} samples at {sample_rate} Hz, outside "
                         f"{MIN_PERIOD}..{MAX_PERIOD}")
    return p_lo, p_hi


def excerpt_range(entry: dict, sample_rate: int) -> tuple[int, int]:
    """(L_lo, L_hi) = (int(lo * sample_rate), int(hi * sample_rate)) of a parsed excerpt entry: samples of the excerpt.
    ValueError unless 1024 <= L_lo <= L_hi <= 2147483520."""
    l_lo, l_hi = int(entry["seconds"][0] * sample_rate), int(entry["seconds"][1] * sample_rate)
    if not MIN_EXCERPT <= l_lo <= l_hi <= 2147483520:
        raise ValueError(f"seconds = {entry['seconds']} is {l_lo}..{l_hi} samples at {sample_rate} Hz; at least {MIN_EXCERPT} "
                         f"are required")
    return l_lo, l_hi


def warp_range(entry: dict, sample_rate: int) -> tuple[int, int, int]:
    """(e_lo, e_hi, D) of a parsed time_warp entry: the breakpoints are 2^e samples apart with e_lo <= e <= e_hi, and a rate is
    (65536 + m) / 65536 with |m| <= D = floor(65536 depth).  A period [lo, hi] in seconds holds the powers of two from
    e_lo = ceil(log2(int(lo * sample_rate))) to e_hi = floor(log2(int(hi * sample_rate))); a scalar v means
    e_lo = e_hi = round(log2(int(v * sample_rate))).  ValueError unless 8 <= e_lo <= e_hi <= 20 and 1 <= D <= 6553."""
    D = int(math.floor(65536.0 * float(entry["depth"])))
    if not 1 <= D <= MAX_WARP_DEPTH:
        raise ValueError(f"depth = {entry['depth']} is a rate offset of {D} / 65536; 1 to {MAX_WARP_DEPTH} are required")
    pd = entry["period"]
    if isinstance(pd, (list, tuple)):
        n_lo, n_hi = int(pd[0] * sample_rate), int(pd[1] * sample_rate)
        e_lo = (n_lo - 1).bit_length() if n_lo >= 1 else -1           # ceil(log2(n_lo)), in integers
        e_hi = n_hi.bit_length() - 1                                   # floor(log2(n_hi)); -1 for no sample at all
    else:
        n_lo = n_hi = int(pd * sample_rate)
        e_lo = e_hi = int(round(math.log2(n_lo))) if n_lo >= 1 else -1
    if not MIN_WARP_EXP <= e_lo <= e_hi <= MAX_WARP_EXP:
        raise ValueError(f"period = {pd} is {n_lo}..{n_hi} samples at {sample_rate} Hz, which holds no power of two from "
                         f"2^{MIN_WARP_EXP} to 2^{MAX_WARP_EXP} (2^{e_lo}..2^{e_hi})")
    return e_lo, e_hi, D


def filter_edge(f: float, sample_rate: int) -> int:
    """c = round(65536 f / sample_rate): a frequency in units of 1 / 65536 cycle per sample."""
    return int(round(65536.0 * float(f) / sample_rate))


def filter_range(entry: dict, sample_rate: int) -> tuple[int, int, int]:
    """(c_lo, c_hi, w_min) of a parsed band_filter entry: its edges' range and a band's least width, through filter_edge."""
    return (filter_edge(entry["freq"][0], sample_rate), filter_edge(entry["freq"][1], sample_rate),
            filter_edge(entry["min_width"], sample_rate))


def shift_increment(hz: float, sample_rate: int) -> int:
    """d = round(hz / sample_rate 2^20): a frequency shift in units of sample_rate / 2^20 Hz, signed."""
    return int(round(float(hz) / sample_rate * PHASE_ONE))


def shift_range(entry: dict, sample_rate: int) -> tuple[int, int]:
    """(d_lo, d_hi) of a parsed frequency_shift entry, through shift_increment.  ValueError unless -65536 <= d_lo <= d_hi <= 65536."""
    d_lo, d_hi = shift_increment(entry["hz"][0], sample_rate), shift_increment(entry["hz"][1], sample_rate)
    if not -MAX_SHIFT <= d_lo <= d_hi <= MAX_SHIFT:
        raise ValueError(f"hz = {entry['hz']} is {d_lo}..{d_hi} in units of {sample_rate} / 2^20 Hz, outside +-{MAX_SHIFT} "
                         f"(+-{sample_rate / 16:g} Hz)")
    return d_lo, d_hi


def filter_mask(entry: dict) -> int:
    """The sum of the bits of a parsed band_filter entry's responses."""
    return sum(RESPONSES[r] for r in entry["response"])


def _clips_longer(head, out_lengths, k, what):
    for b, ny in enumerate(out_lengths):
        if k >= int(ny):
            raise ValueError(head + f"clip {b} has {int(ny)} output samples, not more than the {k} {what}")


def _check_suppression(head, a, sample_rate, out_lengths):
    k = suppression_samples(a, sample_rate)
    if k < 1:
        raise ValueError(head + f"{a['seconds']} s is less than one sample at {sample_rate} Hz")
    _clips_longer(head, out_lengths, k, "to be suppressed")


def _check_reverberation(head, a, sample_rate, out_lengths):
    n_lo, n_hi = reverb_taps(a, sample_rate)
    if n_lo < 2 or n_hi > MAX_IR:
        raise ValueError(head + f"rt60 = {a['rt60']} s is {n_lo}..{n_hi} taps at {sample_rate} Hz, outside 2..{MAX_IR}")


def _check_delete(head, a, sample_rate, out_lengths):
    k_lo, k_hi = delete_range(a, sample_rate)
    if not 1 <= k_lo <= k_hi:
        raise ValueError(head + f"seconds = {a['seconds']} is {k_lo}..{k_hi} samples at {sample_rate} Hz; 1 <= k_lo <= k_hi is required")
    _clips_longer(head, out_lengths, k_hi, "that may be deleted")


def check_lengths(chain: list[dict], sample_rate: int, out_lengths) -> None:
    """ValueError naming the first clip that a suppression would not fit into (0 < k < Ny_b is required), a reverberation
    whose impulse response would have fewer than 2 or more than MAX_IR taps at this sample rate, or a sample deletion without
    1 <= k_lo <= k_hi < Ny_b."""
    for j, a in enumerate(chain):
        if _KIND[a["kind"]].check is not None:
            _KIND[a["kind"]].check(f"loop_attacks[{j}] ({a['kind']}): ", a, sample_rate, out_lengths)


def philox4x32(counter: np.ndarray, key, rounds: int = 10) -> np.ndarray:
    """Philox-4x32 (Salmon et al. 2011) on `counter` [n, 4] uint32 with key (k0, k1); returns [n, 4] uint32."""
    c = np.asarray(counter, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = c[:, 0], c[:, 1], c[:, 2], c[:, 3]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    mask, sh = np.uint64(0xFFFFFFFF), np.uint64(32)
    for _ in range(rounds):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ np.uint64(k0), p1 & mask, (p0 >> sh) ^ c3 ^ np.uint64(k1), p0 & mask
        k0 = (k0 + 0x9E3779B9) & 0xFFFFFFFF
        k1 = (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=1).astype(np.uint32)


def entry_draw(seed: int, step: int, j: int) -> np.ndarray:
    """The four uint32 lanes that decide whether entry j fires at this step (lane 0) and where a suppression starts (lane 1)."""
    return philox4x32(np.array([[0, step, 1 + j, 1]], dtype=np.uint64), (seed, _KEY1))[0]


def fires(r0: int, prob: float) -> bool:
    """(r0 + 0.5) / 2^32 < prob, with prob at the float32 precision the device holds it in."""
    return (float(r0) + 0.5) / 4294967296.0 < float(np.float32(prob))


def suppression_start(r1: int, ny: int, k: int) -> int:
    return (int(r1) * (int(ny) - int(k))) >> 32


def normal_draws(n: int, seed: int, step: int, j: int, word: int = 0) -> np.ndarray:
    """n standard normal draws (float64) of noise entry j at this step: counter (i // 4, step, word, j), key (seed, 0x5EED),
    u = (r + 0.5) / 2^32, z0 = sqrt(-2 ln u0) cos(2 pi u1), z1 = sqrt(-2 ln u0) sin(2 pi u1), z2 / z3 from lanes 2 and 3.
    word 0 is the noise entries' stream; the impulse responses draw from word 8."""
    nblk = (n + 3) // 4
    ctr = np.zeros((nblk, 4), dtype=np.uint64)
    ctr[:, 0] = np.arange(nblk, dtype=np.uint64)
    ctr[:, 1] = step
    ctr[:, 2] = word
    ctr[:, 3] = j
    u = (philox4x32(ctr, (seed, _KEY1)).astype(np.float64) + 0.5) / 4294967296.0
    r0, r1 = np.sqrt(-2.0 * np.log(u[:, 0])), np.sqrt(-2.0 * np.log(u[:, 2]))
    z = np.stack([r0 * np.cos(2 * np.pi * u[:, 1]), r0 * np.sin(2 * np.pi * u[:, 1]),
                  r1 * np.cos(2 * np.pi * u[:, 3]), r1 * np.sin(2 * np.pi * u[:, 3])], axis=1)
    return z.reshape(-1)[:n]


def reverb_length(r2: int, n_lo: int, n_hi: int) -> int:
    """n_h = n_lo + ((r2 * (n_hi - n_lo + 1)) >> 32): uniform on [n_lo, n_hi], in integers as the device computes it."""
    return int(n_lo) + ((int(r2) * (int(n_hi) - int(n_lo) + 1)) >> 32)


def reverb_ir(seed: int, step: int, j: int, n_h: int, drr_db: float) -> np.ndarray:
    """The n_h taps (float64) of entry j's impulse response at this step: an exponentially decaying Gaussian tail that is
    60 dB down at n_h, and a direct path h_0 whose energy is drr_db above the tail's."""
    i = np.arange(n_h, dtype=np.float64)
    h = normal_draws(n_h, int(seed) & 0xFFFFFFFF, step, j, _IR_WORD) * np.exp(-math.log(1000.0) * i / n_h)
    h[0] = 0.0
    h[0] = 10.0 ** (drr_db / 20.0) * math.sqrt(float(np.sum(h * h)))
    return h


def speed_offset(r3: int, m_lo: int, m_hi: int) -> int:
    """m = m_lo + ((r3 * (m_hi - m_lo + 1)) >> 32): uniform on [m_lo, m_hi], in integers as the device computes it."""
    return int(m_lo) + ((int(r3) * (int(m_hi) - int(m_lo) + 1)) >> 32)


def speed_length(n: int, m: int) -> int:
    """Samples of a clip of n played at (65536 + m) / 65536 of its speed: ((n - 1) << 16) // R + 1."""
    return ((int(n) - 1) << 16) // (65536 + int(m)) + 1


def speed_change(x: torch.Tensor, m: int, n_out: int | None = None) -> torch.Tensor:
    """x [..., n] played at R / 65536 of its speed, R = 65536 + m, by Catmull-Rom interpolation at the positions i R in 16.16
    fixed point; n_out samples (default n: the clip keeps its geometry).  Differentiable in x; m = 0 returns x."""
    n = x.shape[-1]
    n_out = n if n_out is None else int(n_out)
    m = int(m)
    if m == 0 and n_out == n:
        return x
    p = np.arange(n_out, dtype=np.int64) * np.int64(65536 + m)
    i0 = p >> 16
    live = p <= (np.int64(n - 1) << 16)
    f = torch.as_tensor((p & 0xFFFF).astype(np.float64) / 65536.0).to(dtype=x.dtype, device=x.device)
    w = (((-f + 2) * f - 1) * f / 2, ((3 * f - 5) * f * f + 2) / 2, ((-3 * f + 4) * f + 1) * f / 2, (f - 1) * f * f / 2)
    z = None
    for t, wt in zip((-1, 0, 1, 2), w):
        idx = i0 + t
        ok = live & (idx >= 0) & (idx < n)
        tap = x[..., torch.as_tensor(np.where(ok, idx, 0), device=x.device)]
        term = wt * tap * torch.as_tensor(ok).to(dtype=x.dtype, device=x.device)
        z = term if z is None else z + term
    return z


def stretch_offset(r3: int, m_lo: int, m_hi: int) -> int:
    """m = m_lo + ((r3 * (m_hi - m_lo + 1)) >> 32): uniform on [m_lo, m_hi], in integers as the device computes it."""
    return int(m_lo) + ((int(r3) * (int(m_hi) - int(m_lo) + 1)) >> 32)


def stretch_length(n: int, m: int) -> int:
    """Samples of a clip of n stretched at the rate (65536 + m) / 65536: ((n - 1) << 16) // Q + 1."""
    return ((int(n) - 1) << 16) // (65536 + int(m)) + 1


def stretch_window() -> np.ndarray:
    """The periodic Hann window of 1024 points in float32, as the loop's STFT holds it."""
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(STRETCH_WIN, dtype=np.float64) / STRETCH_WIN)).astype(np.float32)


def time_stretch(x: torch.Tensor, m: int, n_out: int | None = None) -> torch.Tensor:
    """x [..., n] stretched in time at the rate Q / 65536, Q = 65536 + m (above 1: faster and shorter, at the same pitch), by
    plain overlap-add: z[i] = 1/2 sum_t w[i - t H + 512] x[i - t H + a_t], a_t = (t H Q) >> 16, over the four t (ascending)
    whose window holds i; n_out samples (default n: the clip keeps its geometry).  Linear in x and differentiable; m = 0
    returns x."""
    n = x.shape[-1]
    n_out = n if n_out is None else int(n_out)
    m = int(m)
    if m == 0 and n_out == n:
        return x
    H, N = STRETCH_HOP, STRETCH_WIN
    i = np.arange(n_out, dtype=np.int64)
    w = torch.as_tensor(stretch_window().astype(np.float64)).to(dtype=x.dtype, device=x.device)
    z = None
    for k in (3, 2, 1, 0):                                        # ascending t
        t = (i + N // 2) // H - k                                 # >= -1
        a = (t * np.int64(H) * np.int64(65536 + m)) >> 16         # arithmetic shift
        src = i - t * H + a
        ok = (src >= 0) & (src < n)
        tap = x[..., torch.as_tensor(np.where(ok, src, 0), device=x.device)]
        wk = w[torch.as_tensor(i - t * H + N // 2, device=x.device)] * torch.as_tensor(ok).to(dtype=x.dtype, device=x.device)
        term = wk * tap
        z = term if z is None else z + term
    return 0.5 * z


def pitch_offsets(m: int) -> tuple[int, int]:
    """(R, Q) of a pitch shift at the speed offset m: R = 65536 + m, the ratio the pitch moves by in units of 1 / 65536, and
    the coupled stretch rate Q = ((1 << 32) + R // 2) // R, the nearest integer to 2^32 / R, so that Q R / 2^32 is 1 to within
    2^-17: the stretch lengthens the clip by what the resampling shortens it."""
    R = 65536 + int(m)
    return R, ((1 << 32) + R // 2) // R


def pitch_shift(x: torch.Tensor, m: int, n_out: int | None = None) -> torch.Tensor:
    """x [..., n] with its pitch moved by the ratio R / 65536, R = 65536 + m, at its own duration:
    speed_change(time_stretch(x, mq, L_u), m, n_out) with (R, Q) = pitch_offsets(m), mq = Q - 65536 and the intermediate at its
    true stretched length L_u = stretch_length(n, mq), zero outside; n_out samples (default n).  Linear in x and differentiable;
    m = 0 returns x."""
    n = x.shape[-1]
    n_out = n if n_out is None else int(n_out)
    m = int(m)
    if m == 0 and n_out == n:
        return x
    mq = pitch_offsets(m)[1] - 65536
    return speed_change(time_stretch(x, mq, stretch_length(n, mq)), m, n_out)


def pv_draw(entry: dict, r) -> tuple[int, int]:
    """(mq, m) of a parsed phase_vocoder entry from its draw r = entry_draw(seed, step, j): stretch mode (m = 0) with rate alone,
    or with both keys where r[2] < 2^31; pitch mode otherwise, with the coupled stretch offset mq = pitch_offsets(m)[1] - 65536."""
    if "rate" in entry and ("cents" not in entry or int(r[2]) < (1 << 31)):
        return stretch_offset(r[3], *stretch_range(entry)), 0
    m = speed_offset(r[3], *speed_range(entry))
    return pitch_offsets(m)[1] - 65536, m


def pv_positions(T: int, mq: int):
    """(i, al, live) of the T output frames at Q = 65536 + mq: p = t Q in int64, i = p >> 16, al = (p & 0xFFFF) / 65536 in
    float64 (exact in float32 too), live = i < T."""
    p = np.arange(int(T), dtype=np.int64) * np.int64(65536 + int(mq))
    i = p >> 16
    return i, (p & 0xFFFF).astype(np.float64) / 65536.0, i < int(T)


def _pv_unit(S: torch.Tensor) -> torch.Tensor:
    """u(c) = c / |c|, and 1 for a zero cell: both parts compare equal to 0.  Detached."""
    S = S.detach()
    zero = (S.real == 0) & (S.imag == 0)
    return torch.where(zero, torch.ones_like(S), S / torch.where(zero, torch.ones_like(S.real), S.abs()))


def pv_frames(S: torch.Tensor, mq: int) -> torch.Tensor:
    """The phase vocoder on the frames of a spectrum S [T, F] complex (frame-major, as the device holds it) at the rate
    Q / 65536, Q = 65536 + mq: Y[t] = ((1 - al) |S[i]| + al |S[i + 1]|) P[t], S[T] := 0, Y[t] = 0 where i >= T;
    P[0] = u(S[0]), P[t + 1] = P[t] u(S[i + 1]) conj(u(S[i])).  Differentiable through the magnitudes only (P is detached);
    mq = 0 returns S."""
    mq = int(mq)
    if mq == 0:
        return S
    T = S.shape[0]
    i, al, live = pv_positions(T, mq)
    Sp = torch.cat([S, torch.zeros((2,) + tuple(S.shape[1:]), dtype=S.dtype, device=S.device)])
    U = _pv_unit(Sp)
    ic = np.where(live, i, T)                                         # a dead frame reads the zero rows: magnitude 0, step 1
    i0, i1 = torch.as_tensor(ic, device=S.device), torch.as_tensor(ic + 1, device=S.device)
    step = U[i1] * U[i0].conj()                                       # [T, F]
    P = torch.cat([U[:1], step[:-1]]).cumprod(0)                      # P[t] = u(S[0]) prod_{s < t} step[s]
    a = torch.as_tensor(al, device=S.device).to(S.real.dtype).reshape((-1,) + (1,) * (S.dim() - 1))
    mag = Sp.abs()
    out = ((1 - a) * mag[i0] + a * mag[i1]) * P
    return out * torch.as_tensor(live, device=S.device).to(S.real.dtype).reshape(a.shape)


def _loop_stft(x: torch.Tensor) -> torch.Tensor:
    """The loop's STFT of x [n]: reflect-centred, periodic Hann 1024, hop 256; [n // 256 + 1, 513] complex, frame-major."""
    w = torch.hann_window(STRETCH_WIN, dtype=x.dtype, device=x.device)
    xp = torch.nn.functional.pad(x.reshape(1, 1, -1), (STRETCH_WIN // 2, STRETCH_WIN // 2), mode="reflect").reshape(-1)
    return torch.fft.rfft(xp.unfold(-1, STRETCH_WIN, STRETCH_HOP) * w, dim=-1)


def _loop_istft(Y: torch.Tensor) -> torch.Tensor:
    """The loop's iSTFT of Y [T, 513]: irfft, window, overlap-add, / the squared windows' overlap-add, trimmed to 256 (T - 1)."""
    T = Y.shape[0]
    w = torch.hann_window(STRETCH_WIN, dtype=Y.real.dtype, device=Y.device)
    frames = torch.fft.irfft(Y, n=STRETCH_WIN, dim=-1) * w
    L = STRETCH_WIN + STRETCH_HOP * (T - 1)
    fold = lambda f: torch.nn.functional.fold(f.transpose(0, 1).unsqueeze(0), output_size=(1, L), kernel_size=(1, STRETCH_WIN),
                                              stride=(1, STRETCH_HOP)).reshape(L)
    lo, hi = STRETCH_WIN // 2, STRETCH_WIN // 2 + STRETCH_HOP * (T - 1)
    return fold(frames)[lo:hi] / fold((w * w).expand(T, -1))[lo:hi]


def pv_stretch(x: torch.Tensor, mq: int) -> torch.Tensor:
    """x [n] (n > 512) stretched in time at the rate Q / 65536, Q = 65536 + mq, at its own pitch by the phase vocoder:
    iSTFT(pv_frames(STFT(x), mq)) on the loop's geometry, n samples long (the iSTFT gives 256 (n // 256) of them, zeros follow;
    inside the loop n is a multiple of 256).  Differentiable through the magnitudes; mq = 0 returns x."""
    mq = int(mq)
    if mq == 0:
        return x
    n = x.shape[-1]
    y = _loop_istft(pv_frames(_loop_stft(x), mq))
    return y if y.shape[-1] == n else torch.cat([y, torch.zeros(n - y.shape[-1], dtype=y.dtype, device=y.device)])


def delete_count(r2: int, k_lo: int, k_hi: int) -> int:
    """k = k_lo + ((r2 * (k_hi - k_lo + 1)) >> 32): uniform on [k_lo, k_hi], in integers as the device computes it."""
    return int(k_lo) + ((int(r2) * (int(k_hi) - int(k_lo) + 1)) >> 32)


def delete_draw(entry: dict, r, ny: int, sample_rate: int) -> tuple[int, int]:
    """(start, k) of a parsed delete_samples entry from its draw r = entry_draw(seed, step, j) on a clip of ny samples."""
    k = delete_count(r[2], *delete_range(entry, sample_rate))
    return (suppression_start(r[1], ny, k) if entry["at"] == "anywhere" else 0), k


def delete_samples(x: torch.Tensor, start: int, k: int) -> torch.Tensor:
    """x [..., n] without its samples [start, start + k): z[i] = x[i] for i < start, x[i + k] for start <= i < n - k, 0 behind;
    n samples long.  Differentiable in x (a gather: every value is a copy); k = 0 returns x."""
    n, start, k = x.shape[-1], int(start), int(k)
    if k == 0:
        return x
    if not (0 <= start and 0 < k and start + k <= n):
        raise ValueError(f"delete_samples: the cut [{start}, {start + k}) does not lie inside the {n} samples")
    return torch.cat([x[..., :start], x[..., start + k:], torch.zeros(x.shape[:-1] + (k,), dtype=x.dtype, device=x.device)], dim=-1)


def delete_samples_adjoint(gz: torch.Tensor, start: int, k: int) -> torch.Tensor:
    """The adjoint of delete_samples in gather form: gx[i] = gz[i] for i < start, 0 for start <= i < start + k, gz[i - k] for
    i >= start + k."""
    n, start, k = gz.shape[-1], int(start), int(k)
    if k == 0:
        return gz
    return torch.cat([gz[..., :start], torch.zeros(gz.shape[:-1] + (k,), dtype=gz.dtype, device=gz.device), gz[..., start:n - k]], dim=-1)


def excerpt_draw(entry: dict, r, ny: int, sample_rate: int, on: bool = True) -> tuple[int, int]:
    """(start, L) of a parsed excerpt entry from its draw r = entry_draw(seed, step, j) on a clip of ny samples:
    L = min(L_lo + ((r[2] * (L_hi - L_lo + 1)) >> 32), ny), L = ny where the entry does not fire (on false);
    start = (r[1] * (ny - L + 1)) >> 32."""
    l_lo, l_hi = excerpt_range(entry, sample_rate)
    L = min(l_lo + ((int(r[2]) * (l_hi - l_lo + 1)) >> 32), int(ny)) if on else int(ny)
    return (int(r[1]) * (int(ny) - L + 1)) >> 32, L


def _excerpt_check(n: int, start: int, L: int) -> None:
    if not (0 <= start and 1 <= L and start + L <= n):
        raise ValueError(f"excerpt_tile: the excerpt [{start}, {start + L}) does not lie inside the {n} samples")


def excerpt_tile(x, start, L):
    """z[i] = x[start + (i mod L)], 0 <= i < n: the excerpt [start, start + L) of x repeated periodically until it fills the
    clip.  x a tensor [..., n], or a list of 1-D tensors (ragged) with a start and a length each.  Differentiable in x (a
    gather: every value is a copy); L = n returns x."""
    if not torch.is_tensor(x):
        return [excerpt_tile(xb, s, l) for xb, s, l in zip(x, start, L)]
    n, start, L = x.shape[-1], int(start), int(L)
    _excerpt_check(n, start, L)
    if L == n:
        return x
    return x[..., torch.as_tensor(start + np.arange(n, dtype=np.int64) % L, device=x.device)]


def excerpt_tile_adjoint(gz, start, L):
    """The adjoint of excerpt_tile in gather form: gx[i] = sum_m gz[(i - start) + m L] for start <= i < start + L over
    m = 0, 1, .. while the index is below n, 0 outside.  The sum runs over ascending m in gz's dtype, the first term copied and
    every further one a single rounded addition: in float32 it is the device's, bit for bit.  gz a tensor [..., n] or a
    list of 1-D tensors (ragged) with a start and a length each; L = n returns gz."""
    if not torch.is_tensor(gz):
        return [excerpt_tile_adjoint(gb, s, l) for gb, s, l in zip(gz, start, L)]
    n, start, L = gz.shape[-1], int(start), int(L)
    _excerpt_check(n, start, L)
    if L == n:
        return gz
    acc = gz[..., :L].clone()
    for lo in range(L, n, L):                                         # ascending m: period m covers gz[m L : min((m + 1) L, n)]
        w = min(L, n - lo)
        acc[..., :w] = acc[..., :w] + gz[..., lo:lo + w]
    gx = torch.zeros_like(gz)
    gx[..., start:start + L] = acc
    return gx


def warp_draw(entry: dict, r, sample_rate: int) -> tuple[int, int]:
    """(e, ph) of a parsed time_warp entry from its draw r = entry_draw(seed, step, j): e = e_lo + ((r[2] * (e_hi - e_lo + 1)) >> 32),
    so P = 2^e samples between breakpoints, and ph = (r[1] * P) >> 32 < P the phase of the first."""
    e_lo, e_hi, _ = warp_range(entry, sample_rate)
    e = e_lo + ((int(r[2]) * (e_hi - e_lo + 1)) >> 32)
    return e, (int(r[1]) << e) >> 32


def warp_breakpoints(n: int, e: int) -> int:
    """K = ((n + 2^e - 1) >> e) + 2: the breakpoints a clip of n samples reads at any phase."""
    return ((int(n) + (1 << int(e)) - 1) >> int(e)) + 2


def warp_rates(seed: int, step: int, j: int, n_k: int, D: int) -> np.ndarray:
    """The first n_k rate offsets m_k (int64) of time_warp entry j at this step: w_k = philox4x32_10((k // 4, step, 20 + j, 0),
    (seed, 0x5EED))[k % 4], m_k = -D + ((w_k * (2 D + 1)) >> 32): uniform on [-D, D].  The rate itself is R_k = 65536 + m_k."""
    nblk = (int(n_k) + 3) // 4
    ctr = np.zeros((nblk, 4), dtype=np.uint64)
    ctr[:, 0] = np.arange(nblk, dtype=np.uint64)
    ctr[:, 1] = step
    ctr[:, 2] = _WARP_WORD + int(j)
    w = philox4x32(ctr, (int(seed) & 0xFFFFFFFF, _KEY1)).reshape(-1)[:int(n_k)].astype(np.int64)
    return -int(D) + ((w * np.int64(2 * int(D) + 1)) >> np.int64(32))


def warp_table(rates, e: int) -> tuple[np.ndarray, np.ndarray]:
    """(R, A) of the rate offsets m_k: R_k = 65536 + m_k and A(0) = 0, A(k + 1) = A(k) + P R_k + (((R_{k+1} - R_k) P) >> 1) with
    P = 2^e, both int64 and as long as `rates`: the table the device keeps from the forward pass to the backward pass."""
    R = 65536 + np.asarray(rates, dtype=np.int64)
    P = np.int64(1) << np.int64(e)
    A = np.zeros(len(R), dtype=np.int64)
    if len(R) > 1:
        A[1:] = np.cumsum(P * R[:-1] + (((R[1:] - R[:-1]) * P) >> np.int64(1)))
    return R, A


def warp_positions(n: int, e: int, ph: int, rates) -> np.ndarray:
    """p_i = Pos(i + ph) - Pos(ph), i < n, in int64 (16.16 fixed point) from the rate offsets m_k, at least
    warp_breakpoints(n, e) of them: Pos(u) = A(k) + t R_k + (((R_{k+1} - R_k) t t) >> (e + 1)) with k = u >> e, t = u & (2^e - 1)."""
    n, e, ph = int(n), int(e), int(ph)
    if not (MIN_WARP_EXP <= e <= MAX_WARP_EXP and 0 <= ph < (1 << e)):
        raise ValueError(f"warp_positions: e = {e} outside {MIN_WARP_EXP}..{MAX_WARP_EXP} or ph = {ph} outside [0, 2^e)")
    rates = np.asarray(rates, dtype=np.int64)
    if len(rates) < warp_breakpoints(n, e) or np.any(np.abs(rates) > MAX_WARP_DEPTH):
        raise ValueError(f"warp_positions: {warp_breakpoints(n, e)} rate offsets within +-{MAX_WARP_DEPTH} are required for {n} "
                         f"samples at e = {e}; got {len(rates)}")
    R, A = warp_table(rates, e)
    u = np.concatenate([[0], np.arange(n, dtype=np.int64)]) + np.int64(ph)                 # Pos(ph) first
    k, t = u >> np.int64(e), u & np.int64((1 << e) - 1)
    pos = A[k] + t * R[k] + (((R[k + 1] - R[k]) * t * t) >> np.int64(e + 1))
    return pos[1:] - pos[0]


def _warp_taps(n: int, p: np.ndarray, dtype, device):
    """The four (index, weight) pairs of the Catmull-Rom tap at the positions p on a clip of n samples: index [n_out] int64 with
    the dead taps at 0, weight [n_out] in `dtype`, zero where the tap is dead (outside the clip, or p past its last sample)."""
    i0 = p >> 16
    live = p <= (np.int64(n - 1) << 16)
    f = torch.as_tensor((p & 0xFFFF).astype(np.float64) / 65536.0).to(dtype=dtype, device=device)
    w = (((-f + 2) * f - 1) * f / 2, ((3 * f - 5) * f * f + 2) / 2, ((-3 * f + 4) * f + 1) * f / 2, (f - 1) * f * f / 2)
    out = []
    for t, wt in zip((-1, 0, 1, 2), w):
        idx = i0 + t
        ok = live & (idx >= 0) & (idx < n)
        out.append((torch.as_tensor(np.where(ok, idx, 0), device=device), wt * torch.as_tensor(ok).to(dtype=dtype, device=device)))
    return out


def time_warp(x, e, ph, rates):
    """x played at the moving rate of warp_positions(n, e, ph, rates): z[i] = the speed change's Catmull-Rom tap at p_i, samples
    outside the clip read as zero, zero where p_i lies past the last sample; the clip keeps its length.  x a tensor [..., n],
    or a list of 1-D tensors (ragged) with e, ph and rates each.  Differentiable in x (the rates are numbers, not tensors);
    float32 or float64; rate offsets that are all zero return x."""
    if not torch.is_tensor(x):
        return [time_warp(xb, eb, pb, rb) for xb, eb, pb, rb in zip(x, e, ph, rates)]
    n = x.shape[-1]
    p = warp_positions(n, e, ph, rates)
    if not np.any(np.asarray(rates)[:warp_breakpoints(n, e)]):
        return x
    z = None
    for idx, wt in _warp_taps(n, p, x.dtype, x.device):
        term = wt * x[..., idx]
        z = term if z is None else z + term
    return z


def time_warp_adjoint(gz, e, ph, rates):
    """The adjoint of time_warp: gx[j] = sum over ascending i of w_{j - i0(i)}(f_i) gz[i], in gz's dtype (every tap's
    contributions are added in ascending i, the taps in the order -1, 0, 1, 2).  gz a tensor [..., n] or a list of 1-D tensors
    (ragged) with e, ph and rates each; rate offsets that are all zero return gz."""
    if not torch.is_tensor(gz):
        return [time_warp_adjoint(gb, eb, pb, rb) for gb, eb, pb, rb in zip(gz, e, ph, rates)]
    n = gz.shape[-1]
    p = warp_positions(n, e, ph, rates)
    if not np.any(np.asarray(rates)[:warp_breakpoints(n, e)]):
        return gz
    gx = torch.zeros_like(gz)
    for idx, wt in _warp_taps(n, p, gz.dtype, gz.device):
        gx.index_add_(-1, idx, wt * gz)
    return gx


def envelope_draw(entry: dict, r, sample_rate: int) -> tuple[int, int]:
    """(P, ph) of a parsed gain_envelope entry from its draw r = entry_draw(seed, step, j): P = P_lo + ((r[2] * (P_hi - P_lo + 1))
    >> 32) samples between breakpoints, ph = (r[1] * P) >> 32 < P the phase of the first."""
    p_lo, p_hi = envelope_range(entry, sample_rate)
    P = p_lo + ((int(r[2]) * (p_hi - p_lo + 1)) >> 32)
    return P, (int(r[1]) * P) >> 32


def envelope_gains(seed: int, step: int, j: int, n_k: int, floor: float) -> np.ndarray:
    """The first n_k breakpoint gains (float32) of envelope entry j at this step: w_k = philox4x32_10((k // 4, step, 16 + j, 0),
    (seed, 0x5EED))[k % 4], u_k = (w_k >> 8) 2^-24, g_k = floor + (1 - floor) u_k in float32."""
    nblk = (int(n_k) + 3) // 4
    ctr = np.zeros((nblk, 4), dtype=np.uint64)
    ctr[:, 0] = np.arange(nblk, dtype=np.uint64)
    ctr[:, 1] = step
    ctr[:, 2] = _ENV_WORD + int(j)
    w = philox4x32(ctr, (int(seed) & 0xFFFFFFFF, _KEY1)).reshape(-1)[:int(n_k)]
    u = (w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    fl = np.float32(floor)
    return (fl + (np.float32(1.0) - fl) * u).astype(np.float32)


def envelope_curve(n: int, seed: int, step: int, j: int, P: int, ph: int, floor: float) -> np.ndarray:
    """g(i), i < n, in float32: pos = i + ph, k = pos // P, f = float32(pos - k P) / float32(P), g = g_k + f (g_{k+1} - g_k)."""
    pos = np.arange(int(n), dtype=np.int64) + int(ph)
    k = pos // int(P)
    g = envelope_gains(seed, step, j, (int(k[-1]) + 2) if n else 0, floor)
    f = (pos - k * int(P)).astype(np.float32) / np.float32(P)
    return (g[k] + f * (g[k + 1] - g[k])).astype(np.float32)


def gain_envelope(x, seed, step: int, j: int, P: int, ph: int, floor: float):
    """x * g with g = envelope_curve(...) detached, in x's dtype: x a tensor [n] with one seed, or a list of 1-D tensors (ragged)
    with a seed each.  Differentiable in x; float32 or float64.  Forward and adjoint are the same operator."""
    if not torch.is_tensor(x):
        return [gain_envelope(xb, sd, step, j, P, ph, floor) for xb, sd in zip(x, seed)]
    g = envelope_curve(x.shape[-1], int(seed) & 0xFFFFFFFF, step, j, P, ph, floor)
    return x * torch.as_tensor(g).to(dtype=x.dtype, device=x.device)


def filter_draw(entry: dict, r, sample_rate: int) -> tuple[int, int, int]:
    """(response bit, c1, c2) of a parsed band_filter entry from its draw r = entry_draw(seed, step, j): the edges from r[1] and
    r[2], the response from r[3]; c2 = c1 for lowpass and highpass."""
    c_lo, c_hi, w_min = filter_range(entry, sample_rate)
    e1 = c_lo + ((int(r[1]) * (c_hi - c_lo + 1)) >> 32)
    e2 = c_lo + ((int(r[2]) * (c_hi - c_lo + 1)) >> 32)
    bits = [RESPONSES[n] for n in entry["response"]]
    response = bits[(int(r[3]) * len(bits)) >> 32]
    if response < 4:
        return response, e1, e1
    c1, c2 = min(e1, e2), max(e1, e2)
    return response, c1, max(c2, c1 + w_min)


def _filter_lowpass(c: int, dtype) -> np.ndarray:
    k = np.arange(-FILTER_HALF, FILTER_HALF + 1)
    ak = np.abs(k)
    if dtype == np.float32:
        # the device's arithmetic: the window, the sine of the exact argument, one division
        w = (np.float32(0.54) + np.float32(0.46) * np.cos(np.pi * (ak.astype(np.float32) * np.float32(1.0 / 127.0)).astype(np.float64)).astype(np.float32))
        sn = np.sin(np.pi * ((c * ak) % 65536).astype(np.float64) / 32768.0).astype(np.float32)
        den = (np.float32(np.pi) * np.maximum(ak, 1).astype(np.float32)).astype(np.float32)
        lp = ((w * sn).astype(np.float32) / den).astype(np.float32)
        lp[FILTER_HALF] = np.float32(c) / np.float32(32768.0)
        return lp
    w = 0.54 + 0.46 * np.cos(np.pi * k / FILTER_HALF)
    lp = w * np.sin(2.0 * np.pi * ((c * ak) % 65536) / 65536.0) / (np.pi * np.maximum(ak, 1))
    lp[FILTER_HALF] = c / 32768.0
    return lp


def filter_taps(response: int, c1: int, c2: int, dtype=np.float64) -> np.ndarray:
    """The 255 taps h[k], k = -127..127 at index k + 127, of the response bit (1 lowpass, 2 highpass, 4 bandpass, 8 bandstop) at
    the edges c1 (and c2 for the band responses), in float64 or float32."""
    dtype = np.dtype(dtype).type
    response, c1, c2 = int(response), int(c1), int(c2)
    if response not in RESPONSES.values() or not (0 <= c1 <= MAX_EDGE and 0 <= c2 <= MAX_EDGE):
        raise ValueError(f"filter_taps: response = {response} is not one of 1, 2, 4, 8, or an edge of ({c1}, {c2}) lies outside "
                         f"0..{MAX_EDGE}")
    delta = np.zeros(2 * FILTER_HALF + 1, dtype=dtype)
    delta[FILTER_HALF] = 1
    l1 = _filter_lowpass(c1, dtype)
    if response == 1:
        return l1
    if response == 2:
        return (delta - l1).astype(dtype)
    band = (_filter_lowpass(c2, dtype) - l1).astype(dtype)
    return band if response == 4 else (delta - band).astype(dtype)


def band_filter(x, response, c1, c2):
    """z[i] = sum_k h[k] x[i - k] with h = filter_taps(response, c1, c2) in float64, cast to x's dtype, and x zero outside
    [0, n): x a tensor [..., n], or a list of 1-D tensors (ragged) with a response and edges each.  The clip keeps its length.
    Differentiable in x; the operator is its own adjoint."""
    if not torch.is_tensor(x):
        return [band_filter(xb, rs, a, b) for xb, rs, a, b in zip(x, response, c1, c2)]
    h = torch.as_tensor(filter_taps(response, c1, c2)).to(dtype=x.dtype, device=x.device)
    n = x.shape[-1]
    z = torch.nn.functional.conv1d(x.reshape(-1, 1, n), h.reshape(1, 1, -1), padding=FILTER_HALF)      # h is symmetric: correlation is convolution
    return z.reshape(x.shape)


def shift_draw(entry: dict, r, sample_rate: int) -> tuple[int, int]:
    """(d, p0) of a parsed frequency_shift entry from its draw r = entry_draw(seed, step, j): d = d_lo + ((r[1] * (d_hi - d_lo + 1))
    >> 32), the shift in units of sample_rate / 2^20 Hz, and p0 = r[2] >> 12, the start phase in units of 2^-20 turn."""
    d_lo, d_hi = shift_range(entry, sample_rate)
    return d_lo + ((int(r[1]) * (d_hi - d_lo + 1)) >> 32), int(r[2]) >> 12


def hilbert_taps(dtype=np.float64) -> np.ndarray:
    """The 255 taps h[k], k = -127..127 at index k + 127, of the frequency shift's Hilbert transformer, in float64 or float32:
    w[k] 2 / (pi k) with the band filter's window w[k] = 0.54 + 0.46 cos(pi k / 127) for odd k, exactly 0 for even k."""
    dtype = np.dtype(dtype).type
    k = np.arange(-FILTER_HALF, FILTER_HALF + 1)
    odd = (k & 1) == 1
    if dtype == np.float32:
        # the device's arithmetic: the window, one multiplication by 2, one division
        w = (np.float32(0.54) + np.float32(0.46) * np.cos(np.pi * (np.abs(k).astype(np.float32) * np.float32(1.0 / 127.0)).astype(np.float64)).astype(np.float32))
        den = (np.float32(np.pi) * np.where(odd, k, 1).astype(np.float32)).astype(np.float32)
        return np.where(odd, ((w * np.float32(2.0)).astype(np.float32) / den).astype(np.float32), np.float32(0.0)).astype(np.float32)
    w = 0.54 + 0.46 * np.cos(np.pi * k / FILTER_HALF)
    return np.where(odd, w * 2.0 / (np.pi * np.where(odd, k, 1)), 0.0)


def _shift_phase(n: int, d: int, p0: int, dtype, device):
    """(cos phi_i, sin phi_i), i < n, of phi_i = 2 pi ((p0 + i d) mod 2^20) / 2^20: the phase in integers, the functions in float64."""
    d, p0 = int(d), int(p0)
    if abs(d) > MAX_SHIFT or not 0 <= p0 < PHASE_ONE:
        raise ValueError(f"frequency_shift: d = {d} outside +-{MAX_SHIFT} or p0 = {p0} outside [0, 2^20)")
    phi = 2.0 * np.pi * ((p0 + np.arange(int(n), dtype=np.int64) * d) % PHASE_ONE).astype(np.float64) / PHASE_ONE
    return (torch.as_tensor(np.cos(phi)).to(dtype=dtype, device=device), torch.as_tensor(np.sin(phi)).to(dtype=dtype, device=device))


def _hilbert(x: torch.Tensor) -> torch.Tensor:
    """(Hx)[i] = sum_k h[k] x[i - k] with h = hilbert_taps() in float64, cast to x's dtype, and x zero outside [0, n)."""
    h = torch.as_tensor(hilbert_taps()).to(dtype=x.dtype, device=x.device)
    n = x.shape[-1]
    z = torch.nn.functional.conv1d(x.reshape(-1, 1, n), torch.flip(h, [0]).reshape(1, 1, -1), padding=FILTER_HALF)    # conv1d correlates
    return z.reshape(x.shape)


def frequency_shift(x, d, p0):
    """z[i] = x[i] cos phi_i - (Hx)[i] sin phi_i with phi_i = 2 pi ((p0 + i d) mod 2^20) / 2^20: every component of x moved by
    d sample_rate / 2^20 Hz, upwards for a positive d.  x a tensor [..., n], or a list of 1-D tensors (ragged) with a shift and
    a start phase each.  The clip keeps its length.  Differentiable in x (d and p0 are numbers, not tensors); float32 or float64."""
    if not torch.is_tensor(x):
        return [frequency_shift(xb, db, pb) for xb, db, pb in zip(x, d, p0)]
    cs, sn = _shift_phase(x.shape[-1], d, p0, x.dtype, x.device)
    return x * cs - _hilbert(x) * sn


def frequency_shift_adjoint(gz, d, p0):
    """The adjoint of frequency_shift: gx[j] = gz[j] cos phi_j + (H(gz sin phi))[j], exact because h is antisymmetric and the
    extension is by zeros.  gz a tensor [..., n] or a list of 1-D tensors (ragged) with a shift and a start phase each."""
    if not torch.is_tensor(gz):
        return [frequency_shift_adjoint(gb, db, pb) for gb, db, pb in zip(gz, d, p0)]
    cs, sn = _shift_phase(gz.shape[-1], d, p0, gz.dtype, gz.device)
    return gz * cs + _hilbert(gz * sn)


def _convolve(xb: torch.Tensor, h: np.ndarray) -> torch.Tensor:
    """(h * xb)[0 : len(xb)] in xb's dtype through an FFT at least len(xb) + len(h) - 1 long; differentiable in xb."""
    ny, nh = xb.shape[-1], len(h)
    n = 1 << int(math.ceil(math.log2(ny + nh - 1)))
    ht = torch.as_tensor(h).to(dtype=xb.dtype, device=xb.device)
    return torch.fft.irfft(torch.fft.rfft(xb, n) * torch.fft.rfft(ht, n), n)[..., :ny]


# One operator per kind, apply(xb, a, r, seed, step, j, sample_rate): the parsed entry a at place j of its chain on the clip xb
# with the entry's draw r, at a step where it fires.  The short ones stand in the table itself.
def _apply_noise(xb, a, r, seed, step, j, sample_rate):
    power = float(np.mean(xb.detach().double().cpu().numpy() ** 2))
    sigma = math.sqrt(power / (10.0 ** (a["snr_db"] / 10.0)))
    return xb + torch.as_tensor(sigma * normal_draws(xb.shape[-1], seed, step, j)).to(dtype=xb.dtype, device=xb.device)


def _apply_suppression(xb, a, r, seed, step, j, sample_rate):
    k = suppression_samples(a, sample_rate)
    start = suppression_start(r[1], xb.shape[-1], k)
    mask = torch.ones(xb.shape[-1], dtype=xb.dtype, device=xb.device)
    mask[start:start + k] = 0
    return xb * mask


def _apply_warp(xb, a, r, seed, step, j, sample_rate):
    e, ph = warp_draw(a, r, sample_rate)
    return time_warp(xb, e, ph, warp_rates(seed, step, j, warp_breakpoints(xb.shape[-1], e), warp_range(a, sample_rate)[2]))


# One chain kind: its name and number (AWARE_LOOP_* of include/aware_hip.h), whether it splits the chain, what the one-split
# messages call it, the keys an entry may hold, and its four functions: parse and apply as above, device(a, sample_rate) the
# param[0..3] of the C ABI's aware_loop_attack_ex, check(head, a, sample_rate, out_lengths) the rule of check_lengths, None
# where no rule reads the clips' lengths.
Kind = namedtuple("Kind", "name id splits display keys parse device check apply")


def _kind(name, id, splits, keys, parse, device, check, apply, display=None):
    return Kind(name, id, splits, display or name.replace("_", " "), frozenset(("kind", "prob") + keys), parse, device, check, apply)


# THE TABLE: every kind stated once, in the order of its number.  csrc/loop_limits.hpp holds the device's (kLoopKindTable);
# INTEGRATION.md, "Adding a loop attack kind", lists what else a new kind touches.
TABLE = (
    _kind("gaussian_noise", 0, False, ("snr_db",), _parse_noise, lambda a, sr: [a["snr_db"], 0.0, 0.0, 0.0], None, _apply_noise),
    _kind("sample_suppression", 1, False, ("seconds",), _parse_suppression,
          lambda a, sr: [float(suppression_samples(a, sr)), 0.0, 0.0, 0.0], _check_suppression, _apply_suppression),
    _kind("reverberation", 2, True, ("rt60", "drr_db"), _parse_reverberation,
          lambda a, sr: [*map(float, reverb_taps(a, sr)), a["drr_db"], 0.0], _check_reverberation,
          lambda xb, a, r, seed, step, j, sr: _convolve(xb, reverb_ir(seed, step, j, reverb_length(r[2], *reverb_taps(a, sr)), a["drr_db"]))),
    _kind("speed_change", 3, True, ("cents",), lambda head, a, sr: {"cents": _parse_cents(head, a)},
          lambda a, sr: [*map(float, speed_range(a)), 0.0, 0.0], None,
          lambda xb, a, r, seed, step, j, sr: speed_change(xb, speed_offset(r[3], *speed_range(a)))),
    _kind("time_stretch", 4, True, ("rate",), lambda head, a, sr: {"rate": _parse_rate(head, a)},
          lambda a, sr: [*map(float, stretch_range(a)), 0.0, 0.0], None,
          lambda xb, a, r, seed, step, j, sr: time_stretch(xb, stretch_offset(r[3], *stretch_range(a)))),
    _kind("pitch_shift", 5, True, ("cents",), lambda head, a, sr: {"cents": _parse_cents(head, a)},
          lambda a, sr: [*map(float, speed_range(a)), 0.0, 0.0], None,
          lambda xb, a, r, seed, step, j, sr: pitch_shift(xb, speed_offset(r[3], *speed_range(a)))),
    _kind("phase_vocoder", 6, True, ("rate", "cents"), _parse_vocoder,
          lambda a, sr: [*map(float, stretch_range(a) if "rate" in a else (0, -1)), *map(float, speed_range(a) if "cents" in a else (0, -1))], None,
          lambda xb, a, r, seed, step, j, sr: speed_change(pv_stretch(xb, pv_draw(a, r)[0]), pv_draw(a, r)[1])),
    _kind("delete_samples", 7, True, ("seconds", "at"), _parse_delete,
          lambda a, sr: [*map(float, delete_range(a, sr)), float(DELETE_AT[a["at"]]), 0.0], _check_delete,
          lambda xb, a, r, seed, step, j, sr: delete_samples(xb, *delete_draw(a, r, xb.shape[-1], sr)), display="sample deletion"),
    _kind("gain_envelope", 8, False, ("period", "floor"), _parse_envelope,
          lambda a, sr: [*map(float, envelope_range(a, sr)), a["floor"], 0.0], None,
          lambda xb, a, r, seed, step, j, sr: gain_envelope(xb, seed, step, j, *envelope_draw(a, r, sr), a["floor"])),
    _kind("band_filter", 9, True, ("response", "freq", "min_width"), _parse_filter,
          lambda a, sr: [float(filter_mask(a)), *map(float, filter_range(a, sr))], None,
          lambda xb, a, r, seed, step, j, sr: band_filter(xb, *filter_draw(a, r, sr))),
    _kind("excerpt", 10, True, ("seconds",), lambda head, a, sr: _in_range(head, excerpt_range, {"seconds": _number_or_pair(head, a, "seconds")}, sr),
          lambda a, sr: [*map(float, excerpt_range(a, sr)), 0.0, 0.0], None,
          lambda xb, a, r, seed, step, j, sr: excerpt_tile(xb, *excerpt_draw(a, r, xb.shape[-1], sr)), display="tiled excerpt"),
    _kind("time_warp", 11, True, ("depth", "period"), _parse_warp, lambda a, sr: [*map(float, warp_range(a, sr)), 0.0], None, _apply_warp),
    _kind("frequency_shift", 12, False, ("hz",), _parse_shift, lambda a, sr: [*map(float, shift_range(a, sr)), 0.0, 0.0], None,
          lambda xb, a, r, seed, step, j, sr: frequency_shift(xb, *shift_draw(a, r, sr))),
)
_NAMED = 12                                                    # the kinds the unknown-kind message of parse_chain names
_KIND = {k.name: k for k in TABLE}
KINDS = {k.name: k.id for k in TABLE}                          # AWARE_LOOP_* of include/aware_hip.h
SPLITTING = tuple(k.name for k in TABLE if k.splits)           # the kinds of the one-split rule, in the order of their numbers
# ... and those added since the suite recorded that time_warp is the last of SPLITTING (tests/test_loop_warp_host.py): their rows
# say splits = False, and the one-split rule treats them exactly as the kinds of SPLITTING.  csrc/loop_limits.hpp holds the
# device's list (kLoopStagedBeyond).
STAGED = ("frequency_shift",)


def apply_chain(x, chain, seeds, step: int, sample_rate: int = 16000):
    """The chain on x: a tensor [B, Ny] or a list of B 1-D tensors (ragged), float32 or float64; differentiable (the noise
    amplitude is detached, a suppression multiplies by a 0/1 mask, a gain envelope by its detached gains).  seeds: B integers; step: the optimiser step.  Returns the
    same container type."""
    chain = parse_chain(chain, sample_rate)
    clips = list(x) if not torch.is_tensor(x) else [x[b] for b in range(x.shape[0])]
    if len(seeds) != len(clips):
        raise ValueError(f"apply_chain: {len(clips)} clips but {len(seeds)} seeds")
    check_lengths(chain, sample_rate, [c.shape[-1] for c in clips])
    out = []
    for xb, seed in zip(clips, seeds):
        seed = int(seed) & 0xFFFFFFFF
        for j, a in enumerate(chain):
            r = entry_draw(seed, step, j)
            if fires(r[0], a["prob"]):
                xb = _KIND[a["kind"]].apply(xb, a, r, seed, step, j, sample_rate)
        out.append(xb)
    return torch.stack(out) if torch.is_tensor(x) else out


def device_entries_ex(chain: list[dict], sample_rate: int):
    """(kind, prob, [param0..3]) of the C ABI's aware_loop_attack_ex: kinds 0 and 1 as device_entries in param[0]; a
    reverberation has param = [n_lo, n_hi, drr_db, 0], a speed change, a time stretch or a pitch shift [m_lo, m_hi, 0, 0], a
    phase vocoder [mq_lo, mq_hi, m_lo, m_hi] with [0, -1] (lo > hi) for an absent mode, a sample deletion
    [k_lo, k_hi, at (0 start / 1 anywhere), 0], a gain envelope [P_lo, P_hi, floor, 0], a band filter [mask, c_lo, c_hi, w_min],
    a tiled excerpt [L_lo, L_hi, 0, 0], a time warp [e_lo, e_hi, D, 0], a frequency shift [d_lo, d_hi, 0, 0]."""
    return [(KINDS[a["kind"]], a["prob"], _KIND[a["kind"]].device(a, sample_rate)) for a in chain]


def device_entries(chain: list[dict], sample_rate: int):
    """(kind, param, prob) triples of the C ABI (aware_loop_attack): param = snr_db or the suppression length in samples.
    Chains of these two kinds only; every other kind goes through device_entries_ex."""
    return [(kind_id(a["kind"]), a["snr_db"] if a["kind"] == "gaussian_noise" else float(suppression_samples(a, sample_rate)),
             a["prob"]) for a in chain]


# ---- attack mixtures (EXTENSION): one of several chains drawn per clip and step ---------------------
#
# A chain holds at most one of the kinds that split it, so one chain buys robustness against one family.  A mixture is a list
# of 1..8 chains with weights; at optimiser step s clip b draws r = philox4x32_10((0, s, 12, 1), (seed_b, 0x5EED)) and goes
# through the first chain c with r[0] < T_c, T_c = min(floor((w_0 + .. + w_c) 2^32), 2^32) (the float32 weights summed in
# float64), exactly as under a handle that holds chain c alone; what the weights leave of 1 is the share of clean steps
# (choice -1: the identity).
MAX_CHAINS = 8
_MIX_WORD = 12                  # third Philox counter word of the mixture's draw (0: noise, 1..4: entry draws, 8: responses)


def parse_mixture(mixture) -> list[dict]:
    """Validated copy of a mixture such as [{"weight": 0.5, "chain": [{"kind": "gaussian_noise", "snr_db": 10.0}]}, ...]
    (None / empty: no mixture): a list of {"weight": w, "chain": [...]} with every chain through parse_chain; weight defaults
    to 1 / len(mixture).  ValueError, with the index of the offender: more than eight chains, an entry that is no dict, an
    unknown key, an empty chain, a chain parse_chain refuses, a weight that is negative or not finite, a second chain with a
    reverberation (the handle keeps one set of impulse responses, aware_embed_buffer 13), a weight sum above 1 + 1e-6."""
    if not mixture:
        return []
    if isinstance(mixture, dict) or not isinstance(mixture, (list, tuple)):
        raise ValueError("loop_attack_mixture: a list of {weight: ..., chain: [...]} entries is expected")
    if len(mixture) > MAX_CHAINS:
        raise ValueError(f"loop_attack_mixture: at most {MAX_CHAINS} chains, got {len(mixture)}")
    out, reverb = [], None
    for c, m in enumerate(mixture):
        if not isinstance(m, dict):
            raise ValueError(f"loop_attack_mixture[{c}]: a {{weight: ..., chain: [...]}} entry is expected, got {m!r}")
        extra = set(m) - {"weight", "chain"}
        if extra:
            raise ValueError(f"loop_attack_mixture[{c}]: unknown key(s) {sorted(extra)}")
        try:
            chain = parse_chain(m.get("chain"))
        except ValueError as err:
            raise ValueError(f"loop_attack_mixture[{c}]: {err}") from None
        if not chain:
            raise ValueError(f"loop_attack_mixture[{c}]: the chain is empty")
        try:
            w = float(m.get("weight", 1.0 / len(mixture)))
        except (TypeError, ValueError):
            raise ValueError(f"loop_attack_mixture[{c}]: weight = {m.get('weight')!r} is not a number") from None
        if not (math.isfinite(w) and w >= 0.0):
            raise ValueError(f"loop_attack_mixture[{c}]: weight = {w} has to be finite and >= 0")
        if any(a["kind"] == "reverberation" for a in chain):
            if reverb is not None:
                raise ValueError(f"loop_attack_mixture[{c}]: a second chain with a reverberation (the first is chain {reverb})")
            reverb = c
        out.append({"weight": w, "chain": chain})
    total = float(np.sum(np.asarray([m["weight"] for m in out], dtype=np.float32).astype(np.float64)))
    if total > 1.0 + 1e-6:
        raise ValueError(f"loop_attack_mixture: the weights sum to {total}, above 1")
    return out


def mixture_thresholds(weights) -> list[int]:
    """T_c = min(floor((w_0 + .. + w_c) 2^32), 2^32): the weights at float32, summed in float64 in order."""
    acc, out = 0.0, []
    for w in np.asarray(weights, dtype=np.float32):
        acc += float(w)
        out.append(min(int(math.floor(acc * 4294967296.0)), 1 << 32))
    return out


def mixture_choice(seed: int, step: int, weights) -> int:
    """The chain clip `seed` draws at `step`: the first c with r[0] < T_c, -1 if there is none.  The host twin of
    csrc/loop_mix_kernels.hip."""
    r0 = int(philox4x32(np.array([[0, step, _MIX_WORD, 1]], dtype=np.uint64), (int(seed) & 0xFFFFFFFF, _KEY1))[0][0])
    for c, t in enumerate(mixture_thresholds(weights)):
        if r0 < t:
            return c
    return -1


def mixture_choices(seeds, step: int, weights) -> np.ndarray:
    """mixture_choice for many seeds at once, int32 [len(seeds)]."""
    thr = mixture_thresholds(weights)
    out = np.full(len(seeds), -1, dtype=np.int32)
    for b, seed in enumerate(seeds):            # the key differs per clip, so Philox runs once per seed; the thresholds are shared
        r0 = int(philox4x32(np.array([[0, step, _MIX_WORD, 1]], dtype=np.uint64), (int(seed) & 0xFFFFFFFF, _KEY1))[0][0])
        out[b] = next((c for c, t in enumerate(thr) if r0 < t), -1)
    return out


def mixture_weights(mixture: list[dict]) -> list[float]:
    return [m["weight"] for m in mixture]


def check_mixture_lengths(mixture: list[dict], sample_rate: int, out_lengths) -> None:
    """check_lengths per chain, the offender's index in front."""
    for c, m in enumerate(mixture):
        try:
            check_lengths(m["chain"], sample_rate, out_lengths)
        except ValueError as err:
            raise ValueError(f"loop_attack_mixture[{c}]: {err}") from None


def apply_mixture(x, mixture, seeds, step: int, sample_rate: int = 16000):
    """The mixture on x (container types as apply_chain): per clip, apply_chain of the chain it draws at `step` on that clip
    alone, and the clip itself for choice -1.  Differentiable as apply_chain is."""
    mixture = parse_mixture(mixture)
    clips = list(x) if not torch.is_tensor(x) else [x[b] for b in range(x.shape[0])]
    if len(seeds) != len(clips):
        raise ValueError(f"apply_mixture: {len(clips)} clips but {len(seeds)} seeds")
    check_mixture_lengths(mixture, sample_rate, [c.shape[-1] for c in clips])
    weights = mixture_weights(mixture)
    out = []
    for xb, seed in zip(clips, seeds):
        c = mixture_choice(seed, step, weights)
        out.append(xb if c < 0 else apply_chain([xb], mixture[c]["chain"], [seed], step, sample_rate)[0])
    return torch.stack(out) if torch.is_tensor(x) else out


def device_mixture(mixture: list[dict], sample_rate: int):
    """[(weight, device_entries_ex(chain))] of the C ABI's aware_loop_chain."""
    return [(m["weight"], device_entries_ex(m["chain"], sample_rate)) for m in mixture]
