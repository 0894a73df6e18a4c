"""stft5 (kernel 5 forced) against the oracle on what reordering the frame loop's LDS and store
round trips can get wrong.

The mel rows' stores (mel-128 amp dB, n_fft 2048 / hop 512 and the 48 kHz viewer geometry
win 1920 / hop 480, one block and the default grid), written for a store that waits for the
next frame (measured slower and not kept; the cases hold for any placement of the
store): every row of a stream is written, its last one too, a stream that goes on past its
frames (or past the batch) neither stores again nor loses a row, nothing lands outside the
batch's rows, and no row survives from one launch into the next.

The transposes with both rows of a component in flight at once, the window row read ahead of
the ring insert and the stage-1 twiddles read in rolling batches: the same short tracks through
mel dB, amp dB and complex rows (complex: canonical geometry only), mono and stereo, f32 and s16.

Track lengths: a batch refuses a track shorter than win - 1 samples, as the reference panics
there (lib.rs:413), so no track gives fewer than 4 frames at these geometries and "tracks of 1,
2 and 3 frames" do not exist (test_no_track_below_four_frames). What such tracks would
exercise is reached by the grid instead: with one block (16 streams) the frame sets below make
every stream run exactly 1, then 2, 3, 4 and 8 frames, each cutting tracks in the middle and
crossing their ends; with the default grid every stream ends after one frame.

n_mels not divisible by 4 (the rows whose stores stay immediate): n_mels 126 is accepted by the
plan and runs on kernel 5 (asserted below, not skipped)."""
import ctypes as C

import numpy as np
import pytest

import oracle_ffi as O
from thesia import engine
from tolerances import DB_MAX, DB_P9999, STFT_REL, db_clamped_err, stft_frame_err

pytestmark = pytest.mark.gpu

N_FFT, SR, N_MELS = 2048, 48000, 128
GEOS = [(2048, 512), (1920, 480)]  # (win, hop): the canonical and the viewer instance
GUARD_ROWS = 64
NAN_BITS = np.uint32(0x7FC0DEAD)

# frames per track (a track of f frames: (f - 1) * hop + r samples, r < hop; 4 frames: win - 1)
FRAME_SETS = {
    "one_each": [4, 5, 6],              # 15 frames: one per stream, one stream idle
    "two_each": [4, 5, 6, 5, 6, 5],     # 31: two per stream, the last stream 1 + 1 invalid
    "three_each": [37, 6, 4],           # 47: three per stream, the last stream 2 + 1 invalid
    "four_each": [4, 5, 6, 37],         # 52: four per stream on 13 streams
    "tail": [121],                      # 121: eight per stream, the last stream 1 + 7 invalid
}

_FB = {}
_REF = {}


def _fb(n_mels=N_MELS):
    if n_mels not in _FB:
        _FB[n_mels] = O.calc_mel_fb(SR, N_FFT, n_mels)
    return _FB[n_mels]


def _len_of(frames, win, hop, i):
    return win - 1 if frames == 4 else (frames - 1) * hop + (3 + 7 * i) % hop


def _tracks(lens, channels, fmt, seed):
    rng = np.random.default_rng(seed)
    if fmt == engine.IN_S16:
        return [rng.integers(-30000, 30000, size=(n, channels)).astype(np.int16) for n in lens]
    return [(rng.standard_normal((n, channels)) * 0.3).astype(np.float32) for n in lens]


def _f32(t, fmt):
    return (t.astype(np.float32) / np.float32(32768.0)).astype(np.float32) if fmt == engine.IN_S16 else t


def _mono_fold(t):  # lib.rs:42 channel sum, (0 + c0) + c1 ...
    acc = np.zeros(t.shape[0], np.float32)
    for c in range(t.shape[1]):
        acc = (acc + t[:, c]).astype(np.float32)
    return acc


def _ref(key, tracks, fmt, kind, win, hop, n_mels=N_MELS):
    """The oracle's rows per track, computed once per input set (the key names it)."""
    key = (key, kind, win, hop, n_mels)
    if key not in _REF:
        rows = []
        for t in tracks:
            x = _f32(t, fmt)
            if kind == engine.OUT_COMPLEX:
                rows.append(O.perform_stft(_mono_fold(x), win, hop, N_FFT))
            elif kind == engine.OUT_AMP_DB:
                rows.append(O.track_spec(x, win, hop, N_FFT, O.TRACK_AMP_DB))
            else:
                rows.append(O.track_spec(x, win, hop, N_FFT, O.TRACK_MEL_DB, _fb(n_mels)))
        _REF[key] = rows
    return _REF[key]


def _pack(tracks, channels):
    """tracks one after the other, each starting at a multiple of 2 * channels elements"""
    parts, offs, off = [], [], 0
    for t in tracks:
        gap = (-off) % (2 * channels)
        if gap:
            parts.append(np.zeros(gap, t.dtype))
            off += gap
        offs.append(off)
        parts.append(t.reshape(-1))
        off += t.size
    return np.concatenate(parts), offs


class _Guarded:
    """A batch whose output rows sit between GUARD_ROWS rows of a NaN pattern on either side."""

    def __init__(self, tracks, channels, fmt, kind, win, hop, max_blocks, n_mels=N_MELS):
        mel = kind == engine.OUT_MEL_AMP_DB
        self.plan = engine.Plan(N_FFT, win, hop, kind, sr=SR, n_mels=n_mels if mel else 0)
        flat, offs = _pack(tracks, channels)
        lens = [t.shape[0] for t in tracks]
        self.din = engine.DeviceBuffer.from_host(flat)
        self.T = engine.Batch.frames_for(self.plan, lens)
        self.fl = self.plan.row_bins * (2 if kind == engine.OUT_COMPLEX else 1)
        self.kind = kind
        self.g = GUARD_ROWS * self.fl
        self.dout = engine.DeviceBuffer((self.T * self.fl + 2 * self.g) * 4)
        self.fill()
        ptr = C.c_void_p(self.dout.ptr.value + self.g * 4)
        self.b = engine.Batch(self.plan, self.din, offs, lens, ptr, input_format=fmt, channels=channels,
                              kernel=5, max_blocks=max_blocks)
        assert self.b.kernel == 5
        assert self.b.total_frames == self.T

    def fill(self):
        host = np.full(self.T * self.fl + 2 * self.g, NAN_BITS, np.uint32)
        engine.check(engine.lib.thesia_memcpy_h2d(self.dout.ptr, host.ctypes.data_as(C.c_void_p), host.nbytes))

    def upload(self, tracks, channels):
        flat, _ = _pack(tracks, channels)
        assert flat.nbytes == self.din.nbytes
        engine.check(engine.lib.thesia_memcpy_h2d(self.din.ptr, flat.ctypes.data_as(C.c_void_p), flat.nbytes))

    def run(self):
        """One launch; the rows [T, row floats] after the guards were found untouched and every
        element of the rows written."""
        self.b.run()
        engine.synchronize()
        res = self.dout.to_host(np.uint32)
        g = self.g
        assert np.all(res[:g] == NAN_BITS), "guard rows before the batch were written"
        assert np.all(res[g + self.T * self.fl:] == NAN_BITS), "guard rows after the batch were written"
        rows = res[g:g + self.T * self.fl]
        missing = np.flatnonzero(rows == NAN_BITS)
        assert missing.size == 0, ("elements never written, first rows:", np.unique(missing // self.fl)[:8])
        rows = rows.view(np.float32).reshape(self.T, self.fl)
        return rows.view(np.complex64) if self.kind == engine.OUT_COMPLEX else rows

    def per_track(self, rows):
        f0 = self.b.frame0
        return [rows[int(f0[i]):int(f0[i + 1])] for i in range(len(f0) - 1)]


def _check(tag, kind, outs, refs):
    for i, (got, ref) in enumerate(zip(outs, refs)):
        assert got.shape == ref.shape, (tag, i, got.shape, ref.shape)
        if kind == engine.OUT_COMPLEX:
            err = stft_frame_err(got, ref)
            print(f"{tag} track {i}: rel err {err:.3e}")
            assert err <= STFT_REL, (tag, i, err)
        else:
            mx, p = db_clamped_err(got, ref)
            print(f"{tag} track {i}: dB max err {mx:.4f}, p99.99 {p:.4f}")
            assert mx <= DB_MAX and p <= DB_P9999, (tag, i, mx, p)
            assert np.isfinite(got).all()


@pytest.mark.parametrize("win,hop", GEOS)
def test_no_track_below_four_frames(win, hop):
    # the shortest track a batch takes (win - 1 samples) gives 4 frames; one sample less is refused
    plan = engine.Plan(N_FFT, win, hop, engine.OUT_MEL_AMP_DB, sr=SR, n_mels=N_MELS)
    assert engine.Batch.frames_for(plan, [win - 1]) == 4
    assert engine.Batch.frames_for(plan, [win - 2]) == 0
    din = engine.DeviceBuffer(4 * win * 2)
    dout = engine.DeviceBuffer(16 * N_MELS * 4)
    with pytest.raises(Exception):
        engine.Batch(plan, din, [0], [win - 2], dout, input_format=engine.IN_F32, channels=2)


@pytest.mark.parametrize("max_blocks", [1, 0])
@pytest.mark.parametrize("win,hop", GEOS)
@pytest.mark.parametrize("name", list(FRAME_SETS))
def test_held_row_is_stored_once_and_in_place(name, win, hop, max_blocks):
    frames = FRAME_SETS[name]
    lens = [_len_of(f, win, hop, i) for i, f in enumerate(frames)]
    tracks = _tracks(lens, 2, engine.IN_F32, 100 + len(frames))
    gb = _Guarded(tracks, 2, engine.IN_F32, engine.OUT_MEL_AMP_DB, win, hop, max_blocks)
    assert gb.T == sum(frames)
    if name != "one_each":
        assert gb.T % 16 != 0  # one block: 16 streams
    outs = gb.per_track(gb.run())
    assert [len(o) for o in outs] == frames
    _check((name, win, max_blocks), engine.OUT_MEL_AMP_DB, outs,
           _ref(name, tracks, engine.IN_F32, engine.OUT_MEL_AMP_DB, win, hop))


@pytest.mark.parametrize("max_blocks", [1, 0])
@pytest.mark.parametrize("win,hop", GEOS)
def test_second_launch_shows_nothing_of_the_first(win, hop, max_blocks):
    frames = FRAME_SETS["three_each"]
    lens = [_len_of(f, win, hop, i) for i, f in enumerate(frames)]
    first = _tracks(lens, 2, engine.IN_F32, 200)
    second = _tracks(lens, 2, engine.IN_F32, 201)
    gb = _Guarded(first, 2, engine.IN_F32, engine.OUT_MEL_AMP_DB, win, hop, max_blocks)
    rows1 = gb.run().copy()
    gb.fill()
    gb.upload(second, 2)
    rows2 = gb.run().copy()
    fresh = _Guarded(second, 2, engine.IN_F32, engine.OUT_MEL_AMP_DB, win, hop, max_blocks).run()
    assert np.array_equal(rows2.view(np.uint32), fresh.view(np.uint32))
    # (different noise: no row of the second launch equals the first launch's row at its place)
    assert not np.any(np.all(rows1.view(np.uint32) == rows2.view(np.uint32), axis=1))
    _check(("second", win, max_blocks), engine.OUT_MEL_AMP_DB, gb.per_track(rows2),
           _ref("second", second, engine.IN_F32, engine.OUT_MEL_AMP_DB, win, hop))


@pytest.mark.parametrize("max_blocks", [1, 0])
@pytest.mark.parametrize("win,hop", GEOS)
def test_n_mels_not_a_multiple_of_four(win, hop, max_blocks):
    # rows of 126 floats: no 16-byte row stores, the stores stay where they were
    n_mels = 126
    assert _fb(n_mels).shape == (N_FFT // 2 + 1, n_mels)
    frames = FRAME_SETS["three_each"]
    lens = [_len_of(f, win, hop, i) for i, f in enumerate(frames)]
    tracks = _tracks(lens, 2, engine.IN_F32, 300)
    gb = _Guarded(tracks, 2, engine.IN_F32, engine.OUT_MEL_AMP_DB, win, hop, max_blocks, n_mels=n_mels)
    assert gb.plan.row_bins == n_mels and gb.b.kernel == 5
    _check(("mels126", win, max_blocks), engine.OUT_MEL_AMP_DB, gb.per_track(gb.run()),
           _ref("mels126", tracks, engine.IN_F32, engine.OUT_MEL_AMP_DB, win, hop, n_mels))


_KINDS = [(engine.OUT_MEL_AMP_DB, 2048, 512), (engine.OUT_MEL_AMP_DB, 1920, 480),
          (engine.OUT_AMP_DB, 2048, 512), (engine.OUT_AMP_DB, 1920, 480),
          (engine.OUT_COMPLEX, 2048, 512)]


@pytest.mark.parametrize("channels,fmt", [(1, engine.IN_F32), (2, engine.IN_F32), (1, engine.IN_S16),
                                          (2, engine.IN_S16)])
@pytest.mark.parametrize("kind,win,hop", _KINDS)
def test_transposes_every_kind_and_input(kind, win, hop, channels, fmt):
    # one block: a few frames per stream, tracks cut in the middle and crossed at their ends
    lens = [win - 1, 5000, 36 * hop + 7]
    tracks = _tracks(lens, channels, fmt, 400 + 10 * channels + fmt)
    gb = _Guarded(tracks, channels, fmt, kind, win, hop, 1)
    _check((kind, win, channels, fmt), kind, gb.per_track(gb.run()),
           _ref(("short3", channels, fmt), tracks, fmt, kind, win, hop))
