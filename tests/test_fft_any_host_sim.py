"""CPU tests of the general-geometry STFT path (no GPU): the lane simulation of the general-size wave FFT
(aware_amd/csrc/fft_any.hpp) against a double-precision DFT, the NOLA decision against torch.istft, and the refusals of
unsupported geometries."""
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT


def test_fft_any_host_simulation(tmp_path):
    src = os.path.join(ROOT, "tests", "host_sim", "fft_any_sim.cpp")
    exe = str(tmp_path / "fft_any_sim")
    subprocess.run(["hipcc", "-O2", "-x", "hip", "--offload-host-only", "-o", exe, src], check=True)
    lines = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.strip().splitlines()
    sizes = set()
    for line in lines:
        tok = line.split()
        vals = dict(zip(tok[0::2], map(float, tok[1::2])))
        n = int(vals["N"])
        sizes.add(n)
        assert vals["rfft_maxerr"] / vals["rfft_maxmag"] <= 5e-7, line
        assert vals["irfft_maxerr"] <= 1e-6, line
    assert sizes == {256, 512, 1024, 2048, 4096}


def _torch_istft_raises(n_fft, hop, win, window, T):
    w = (torch.hann_window if window == "hann" else torch.hamming_window)(win, dtype=torch.float64)
    X = torch.ones(n_fft // 2 + 1, T, dtype=torch.complex128)
    try:
        torch.istft(X, n_fft, hop, win, w, center=True)
    except RuntimeError as e:
        # (torch.istft also refuses hop > win_length up front; such a window leaves gaps, i.e. a zero envelope)
        assert "window overlap add min" in str(e) or "hop_length <= win_length" in str(e), e
        return True
    return False


def _grid():
    out = []
    for n_fft in (256, 1024, 4096):
        hops = sorted({n_fft // 8, n_fft // 4, n_fft // 2, n_fft, 3 * n_fft // 8 + 1})
        wins = sorted({n_fft, n_fft // 2, n_fft // 4, n_fft // 2 + 1})
        for hop in hops:
            for win in wins:
                for window in ("hann", "hamming"):
                    out.append((n_fft, hop, win, window))
    return out


def test_nola_decision_matches_torch_istft():
    from aware_amd import runtime as rt
    raised = 0
    for n_fft, hop, win, window in _grid():
        for n in (n_fft // 2 + 1 + hop, 3 * n_fft + 17):
            T = 1 + n // hop
            if T < 2:
                continue
            expect_raise = _torch_istft_raises(n_fft, hop, win, window, T)
            raised += expect_raise
            assert rt.nola_ok(n_fft, hop, win, window, n) == (not expect_raise), (n_fft, hop, win, window, n)
    assert raised > 0          # the grid covers refused geometries (e.g. hann, win 256 at n_fft 1024, hop 512)
    assert not rt.nola_ok(1024, 512, 256, "hann", 16000)


@pytest.mark.parametrize("n_fft", [768, 8192])
def test_plugins_refuse_unsupported_n_fft(n_fft):
    from aware_amd.utils.audio import STFT, ISTFT
    for cls in (STFT, ISTFT):
        with pytest.raises(NotImplementedError, match="256, 512, 1024, 2048, 4096"):
            cls(n_fft, n_fft // 4, "hann", n_fft)


def test_plugins_validate_hop_and_win_length():
    from aware_amd.utils.audio import STFT
    for hop, win in ((0, 1024), (1025, 1024), (256, 0), (256, 1025)):
        with pytest.raises(ValueError):
            STFT(1024, hop, "hann", win)
    with pytest.raises(ValueError):
        STFT(1024, 256, "blackman", 1024)


@pytest.mark.parametrize("geom", [(2048, 512, 2048), (1024, 256, 512), (1024, 128, 1024)])
def test_embedder_and_detector_refuse_non_card_geometry(geom):
    """The embed / detect loop runs on the card geometry only: a non-card frame_length / hop_length / win_length is
    refused at construction, before any plan exists (win_length used to be dropped silently)."""
    from aware_amd.embedding import AWAREEmbedder
    from aware_amd.detection import AWAREDetector
    n_fft, hop, win = geom
    with pytest.raises(NotImplementedError, match="model card"):
        AWAREEmbedder(frame_length=n_fft, hop_length=hop, win_length=win)
    with pytest.raises(NotImplementedError, match="model card"):
        AWAREDetector(None, frame_length=n_fft, hop_length=hop, win_length=win)


def test_general_entry_points_declared():
    from aware_amd._lib import load_library
    lib = load_library()
    assert lib.aware_version() >= 310
    assert lib.aware_nola_check(768, 256, 768, 0, 4096) == -2
    assert lib.aware_nola_check(1024, 0, 1024, 0, 4096) == -1
    assert lib.aware_nola_check(1024, 256, 1024, 0, 4096) == 0
