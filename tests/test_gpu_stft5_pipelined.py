"""stft5's mel instances (kernel 5, mel-128 amp dB; n_fft 2048 / hop 512, and the 48 kHz viewer
geometry win 1920 / hop 480, whose instance runs the same mel stream) against the oracle on the
shapes where the streamed frame loop and the read-ahead of the packed mel stream can go
wrong: tracks so short that no frame is on the fast path, streams cut in the middle of a track
and crossing track ends right after a fast-path frame, a misaligned track (its hops are never
prefetched), a frame count that is no multiple of the stream count (invalid tail iterations),
and two grids on the same input, whose outputs must be identical although their stream cuts
differ."""
import numpy as np
import pytest

import oracle_ffi as O
from thesia import engine
from tolerances import DB_MAX, DB_P9999, db_clamped_err

pytestmark = pytest.mark.gpu

N_FFT, HOP, SR, N_MELS = 2048, 512, 48000, 128
GEOS = [(2048, 512), (1920, 480)]  # (win, hop): the canonical and the viewer instance

_FB = {}
_REF = {}


def _fb():
    if "fb" not in _FB:
        _FB["fb"] = O.calc_mel_fb(SR, N_FFT, N_MELS)
    return _FB["fb"]


def _tracks(lens, channels, fmt, seed):
    rng = np.random.default_rng(seed)
    if fmt == engine.IN_S16:
        return [rng.integers(-30000, 30000, size=(n, channels)).astype(np.int16) for n in lens]
    return [(rng.standard_normal((n, channels)) * 0.3).astype(np.float32) for n in lens]


def _ref(key, tracks, fmt, win=N_FFT, hop=HOP):
    """The oracle's mel dB rows per track, computed once per input set (the key names it)."""
    if key not in _REF:
        rows = []
        for t in tracks:
            x = (t.astype(np.float32) / np.float32(32768.0)).astype(np.float32) if fmt == engine.IN_S16 else t
            rows.append(O.track_spec(x, win, hop, N_FFT, O.TRACK_MEL_DB, _fb()))
        _REF[key] = rows
    return _REF[key]


def _run(tracks, channels, fmt, odd, max_blocks, win=N_FFT, hop=HOP):
    """tracks packed one after the other, each starting at a multiple of 2 * channels elements
    (the streaming loads' alignment), plus one element where odd[i]: that track is misaligned."""
    parts, offs, off = [], [], 0
    for t, o in zip(tracks, odd):
        gap = (-off) % (2 * channels) + (1 if o else 0)
        if gap:
            parts.append(np.zeros(gap, t.dtype))
            off += gap
        offs.append(off)
        parts.append(t.reshape(-1))
        off += t.size
    plan = engine.Plan(N_FFT, win, hop, engine.OUT_MEL_AMP_DB, sr=SR, n_mels=N_MELS)
    lens = [t.shape[0] for t in tracks]
    din = engine.DeviceBuffer.from_host(np.concatenate(parts))
    T = engine.Batch.frames_for(plan, lens)
    dout = engine.DeviceBuffer(T * plan.row_bins * 4)
    b = engine.Batch(plan, din, offs, lens, dout, input_format=fmt, channels=channels, kernel=5,
                     max_blocks=max_blocks)
    assert b.kernel == 5
    b.run()
    engine.synchronize()
    out = dout.to_host(np.float32, (T, plan.row_bins))
    return out, [out[int(b.frame0[i]):int(b.frame0[i + 1])] for i in range(len(tracks))]


def _check(key, tracks, fmt, outs, win=N_FFT, hop=HOP):
    for t, got, ref in zip(tracks, outs, _ref(key, tracks, fmt, win, hop)):
        assert got.shape == ref.shape, (len(t), got.shape, ref.shape)
        mx, p = db_clamped_err(got, ref)
        print(f"{key} n={len(t)}: dB max err {mx:.4f}, p99.99 {p:.4f}")
        assert mx <= DB_MAX and p <= DB_P9999, (len(t), mx, p)
        assert np.isfinite(got).all()


@pytest.mark.parametrize("max_blocks", [1, 0])
def test_short_tracks_never_on_the_fast_path(max_blocks):
    # 4-9 frames per track, each reflect-padded or the last of its track: every frame is loaded
    # whole, none from the ring
    lens = [2047, 2048, 2560, 4097]
    tracks = _tracks(lens, 2, engine.IN_F32, 1)
    _, outs = _run(tracks, 2, engine.IN_F32, [0] * 4, max_blocks)
    _check("short", tracks, engine.IN_F32, outs)


_LENS3 = [5000, 7777, 12345]


@pytest.mark.parametrize("channels,fmt", [(1, engine.IN_F32), (2, engine.IN_F32), (1, engine.IN_S16),
                                          (2, engine.IN_S16)])
@pytest.mark.parametrize("odd", [0, 1])
@pytest.mark.parametrize("win,hop", GEOS)
def test_stream_cuts_track_ends_and_misalignment(channels, fmt, odd, win, hop):
    # one block: 16 streams of a few frames each cut the tracks in the middle and cross their
    # ends right after fast-path frames; every track starts aligned, except that with odd the
    # second one starts one element later (no prefetch anywhere in it)
    tracks = _tracks(_LENS3, channels, fmt, 10 + channels)
    _, outs = _run(tracks, channels, fmt, [0, odd, 0], 1, win, hop)
    _check(("three", channels, fmt, win), tracks, fmt, outs, win, hop)


@pytest.mark.parametrize("channels,fmt", [(2, engine.IN_F32), (1, engine.IN_S16)])
@pytest.mark.parametrize("win,hop", GEOS)
def test_grids_agree_bit_for_bit(channels, fmt, win, hop):
    # the stream cuts of one block and of the default grid differ, so different frames come
    # from the ring and from whole loads: the rows must not depend on it
    tracks = _tracks(_LENS3 + [40 * hop + 5], channels, fmt, 20 + channels)
    one, outs = _run(tracks, channels, fmt, [0] * 4, 1, win, hop)
    dflt, _ = _run(tracks, channels, fmt, [0] * 4, 0, win, hop)
    assert np.array_equal(one.view(np.uint32), dflt.view(np.uint32))
    _check(("grids", channels, fmt, win), tracks, fmt, outs, win, hop)


@pytest.mark.parametrize("win,hop", GEOS)
def test_invalid_tail_after_streamed_frames(win, hop):
    # 121 frames on one block's 16 streams (8 frames each): the last stream runs 7 iterations
    # past the end of the batch after frames that were streamed
    tracks = _tracks([120 * hop + 9], 2, engine.IN_F32, 30)
    out, outs = _run(tracks, 2, engine.IN_F32, [0], 1, win, hop)
    assert out.shape[0] == 121 and out.shape[0] % 16 != 0
    _check(("tail", win), tracks, engine.IN_F32, outs, win, hop)


@pytest.mark.parametrize("n_mels", [64, 96, 128])
@pytest.mark.parametrize("mel_path", [2, 3])
def test_chunk_counts_and_steps(n_mels, mel_path):
    # the packed stream built for 2 and for 3 float4 steps per chunk, and filter banks whose
    # chunk counts differ: the read-ahead's tail (chunks left over after the rounds of three)
    # and its clamped reads past the last chunk take every form
    tracks = _tracks([12345], 2, engine.IN_F32, 40)
    plan = engine.Plan(N_FFT, N_FFT, HOP, engine.OUT_MEL_AMP_DB, sr=SR, n_mels=n_mels)
    din = engine.DeviceBuffer.from_host(tracks[0].reshape(-1))
    T = engine.Batch.frames_for(plan, [12345])
    dout = engine.DeviceBuffer(T * plan.row_bins * 4)
    b = engine.Batch(plan, din, [0], [12345], dout, input_format=engine.IN_F32, channels=2, kernel=5,
                     max_blocks=1, mel_path=mel_path)
    assert b.kernel == 5
    b.run()
    engine.synchronize()
    got = dout.to_host(np.float32, (T, plan.row_bins))
    ref = O.track_spec(tracks[0], N_FFT, HOP, N_FFT, O.TRACK_MEL_DB, O.calc_mel_fb(SR, N_FFT, n_mels))
    mx, p = db_clamped_err(got, ref)
    print(f"n_mels {n_mels} mel_path {mel_path}: dB max err {mx:.4f}, p99.99 {p:.4f}")
    assert got.shape == ref.shape and mx <= DB_MAX and p <= DB_P9999, (mx, p)
