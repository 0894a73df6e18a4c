"""Parity on the exact measured configurations and end to end.

  bench   the headline bench line's own workload and kernel: stft5_kernel on stereo f32
          interleaved tracks from the device generator bench.py uses (whose bytes must equal its
          host twin), 30 s tracks, mel-128 amp dB vs the oracle (lib.rs:112-136).
  C1      BASELINE.json configs[0]: the 48 kHz sample substitute (tests/fixtures.py), n_fft 1024
          / hop 256 / Hann, |X| (lib.rs:124) vs the oracle, the whole 2 113 529-sample track.
  E2E     PCM -> the oracle's full pipeline (STFT, |X| [, mel], dB, global range lib.rs:194-209,
          spec_to_grey display.rs:44-54, Lanczos3 + colormap display.rs:56-61) against the
          device's RGB bytes: SURVEY.md §8c (iv) allows <= 1 LSB on <= 1e-4 of the pixels.
"""
import numpy as np
import pytest

import fixtures
import oracle_ffi as O
import thesia
from thesia import engine, pipeline, shard
from tolerances import DB_MAX, DB_P9999, db_clamped_err

pytestmark = pytest.mark.gpu

E2E_MAX_LSB = 1
E2E_MAX_FRAC = 1e-4
# fixed caps of the fast path's e2e contract (_check_multitrack), beside its fixture-relative
# bounds: 2.5e-4 of the pixels (the oracle's own flip share against float64 on the linear
# excerpts is 1.15e-4, so its relative bound reaches 2.3e-4) and 1 dB on the global min
E2E_FLIP_CAP = 2.5e-4
E2E_GMIN_CAP_DB = 1.0


def _rgb_diff(got: np.ndarray, ref: np.ndarray):
    """(max |diff| over channels, fraction of pixels with any channel differing)."""
    d = np.abs(got.reshape(-1, 3).astype(np.int16) - ref.reshape(-1, 3).astype(np.int16))
    per_px = d.max(axis=1)
    return int(per_px.max(initial=0)), float((per_px > 0).mean()) if per_px.size else 0.0


def test_bench_config_exact():
    """bench.py's C4 shard configuration on 3 of its tracks: same generator call, same layout,
    same plan, same kernel."""
    n_tracks, n, sr, ch = 3, 1_440_000, 48000, 2
    din = engine.DeviceBuffer(n_tracks * n * ch * 4)
    engine.synth_pcm_device(din, engine.IN_F32, ch, n_tracks, n, sr, seed=0)
    dev_pcm = din.to_host(np.float32, (n_tracks, n, ch))
    plan = engine.Plan(2048, 2048, 512, engine.OUT_MEL_AMP_DB, sr=sr, n_mels=128)
    offs = np.arange(n_tracks, dtype=np.uint64) * (n * ch)
    T = engine.Batch.frames_for(plan, [n] * n_tracks)
    assert T == 2813 * n_tracks
    dout = engine.DeviceBuffer(T * 128 * 4)
    b = engine.Batch(plan, din, offs, [n] * n_tracks, dout, input_format=engine.IN_F32, channels=ch)
    assert b.kernel == 5  # the bench's kernel (stft5_kernel, the n_fft 2048 default)
    b.run()
    engine.synchronize()
    got = dout.to_host(np.float32, (T, 128))
    fb = O.calc_mel_fb(sr, 2048, 128)
    for k in range(n_tracks):
        host = fixtures.s16_to_f32(engine.synth_pcm_host(ch, k, n, sr, seed=0))
        assert np.array_equal(dev_pcm[k].view(np.uint32), host.view(np.uint32)), k  # generator twin
        ref = O.track_spec(host, 2048, 512, 2048, O.TRACK_MEL_DB, fb)
        mx, p = db_clamped_err(got[2813 * k:2813 * (k + 1)], ref)
        assert mx <= DB_MAX and p <= DB_P9999, (k, mx, p)
    assert np.isfinite(got).all()


def test_c1_48k_substitute_1024_256_magnitude():
    x = fixtures.s16_to_f32(fixtures.c1_substitute())
    n = x.shape[0]
    plan = engine.Plan(1024, 1024, 256, engine.OUT_MAG, sr=48000)
    din = engine.DeviceBuffer.from_host(x)
    T = engine.Batch.frames_for(plan, [n])
    assert T == 8256
    dout = engine.DeviceBuffer(T * 513 * 4)
    b = engine.Batch(plan, din, [0], [n], dout)
    assert b.kernel == 3
    b.run()
    engine.synchronize()
    got = dout.to_host(np.float32, (T, 513))
    ref = O.norm(O.perform_stft(x, 1024, 256, 1024))
    scale = np.abs(ref).max(axis=1, keepdims=True)
    err = np.abs(got - ref) / np.maximum(scale, 1e-30)
    assert float(err.max()) <= 4e-6, float(err.max())  # |X| within the STFT contract (2e-6 x 2)


def _oracle_amp_db(t):
    x = (np.float32(0.0) + fixtures.s16_to_f32(t.pcm)).astype(np.float32)  # lib.rs:42 fold
    return O.track_spec(x, t.n_fft, t.n_fft // 4, t.n_fft, O.TRACK_AMP_DB)


def test_e2e_rgb_c5_generator():
    """Mixed rates and n_fft (the C5 generator): device RGB vs the all-oracle pipeline from
    the same PCM (the oracle's own dB, the oracle's own global range)."""
    tracks = pipeline.c5_tracks(12, seconds=2.0)
    nh = 200
    out = pipeline.render_tracks(tracks, px_per_sec=100.0, nheight=nh)
    ref_db = [_oracle_amp_db(t) for t in tracks]
    gmax, gmin, max_sr = shard.global_db_range(max(float(d.max()) for d in ref_db),
                                               min(float(d.min()) for d in ref_db),
                                               max(t.sr for t in tracks))
    worst, diff_px, total_px = 0, 0.0, 0
    for t, r, db in zip(tracks, out, ref_db):
        grey = O.spec_to_grey(db, shard.up_ratio(t.sr, max_sr, freq_scale_mel=False), gmax, gmin)
        img, _ = O.grey_to_rgb(grey, r.nwidth, nh)
        m, f = _rgb_diff(r.rgb, img)
        worst = max(worst, m)
        diff_px += f * img.size / 3
        total_px += img.size // 3
    assert worst <= E2E_MAX_LSB and diff_px / total_px <= E2E_MAX_FRAC, (worst, diff_px, total_px)


@pytest.mark.parametrize("kernel", [7, 9])
def test_e2e_rgb_c5_generator_exact(kernel):
    """The C5 generator through the reference-order kernels (7: the streaming stftr / stftq, 9:
    stftx): the device RGB bytes equal the all-oracle pipeline's, every pixel of every track
    (north_star: bit-exact for the final u8 buffer), n_fft 256 / 512 / 1024 / 2048 at six rates."""
    tracks = pipeline.c5_tracks(12, seconds=2.0)
    nh = 200
    out = pipeline.render_tracks(tracks, px_per_sec=100.0, nheight=nh, kernel=kernel)
    ref_db = [_oracle_amp_db(t) for t in tracks]
    gmax, gmin, max_sr = shard.global_db_range(max(float(d.max()) for d in ref_db),
                                               min(float(d.min()) for d in ref_db),
                                               max(t.sr for t in tracks))
    for i, (t, r, db) in enumerate(zip(tracks, out, ref_db)):
        grey = O.spec_to_grey(db, shard.up_ratio(t.sr, max_sr, freq_scale_mel=False), gmax, gmin)
        img, _ = O.grey_to_rgb(grey, r.nwidth, nh)
        assert np.array_equal(np.asarray(r.rgb, np.uint8).reshape(-1), np.asarray(img, np.uint8).reshape(-1)), \
            (i, t.sr, t.n_fft, _rgb_diff(r.rgb, img))


def _oracle_specs(pcm, srs, scale, with_f64=False):
    """Per track: the oracle's amp-dB rows (|X| [, mel], dB; lib.rs:112-136) and, with_f64, the
    same rows from the float64 spectrum (tolerances.stft_f64), i.e. what both the reference's f32
    path and the kernels approximate. A thread pool (the oracle's C calls release the GIL)."""
    from concurrent.futures import ThreadPoolExecutor
    from tolerances import stft_f64
    mel = scale == thesia.FreqScale.Mel

    def spec(args):
        x, sr = args
        win, hop, n_fft = O.track_params(sr)
        w = (O.hann(win) / np.float32(n_fft)).astype(np.float32)
        x = (np.float32(0.0) + x).astype(np.float32)
        mag = O.norm(O.perform_stft(x, win, hop, n_fft, window=w))
        fb = O.calc_mel_fb_default(sr, n_fft) if mel else None
        if mel:
            mag = O.dot(mag, fb)
        db64 = None
        if with_f64:
            m64 = np.abs(stft_f64(x, win, hop, n_fft, w))
            if mel:
                m64 = m64 @ fb.astype(np.float64)
            db64 = (20.0 * np.log10(np.maximum(m64, 1e-18))).astype(np.float32)
        return O.amp_to_db_default(mag), db64

    with ThreadPoolExecutor(min(16, len(pcm))) as ex:
        res = list(ex.map(spec, zip(pcm, srs)))
    return [r[0] for r in res], [r[1] for r in res]


def _global_range(dbs, db_range=120.0):
    """lib.rs:194-209 (in f32)."""
    gmax = float(np.float32(min(max(float(d.max()) for d in dbs), 0.0)))
    gmin = float(np.float32(max(min(float(d.min()) for d in dbs), gmax - db_range)))
    return gmax, gmin


def _oracle_images(pcm, srs, scale, nh, dbs, rng):
    """spec_to_grey (display.rs:44-54) + Lanczos3 + colormap (display.rs:56-61) of the given dB
    rows under the given global range, the reference's geometry (lib.rs:231-248, 294-298)."""
    from concurrent.futures import ThreadPoolExecutor
    mel = scale == thesia.FreqScale.Mel
    gmax, gmin = rng

    def one(args):
        x, sr, db = args
        up = shard.up_ratio(sr, max(srs), freq_scale_mel=mel)
        grey = O.spec_to_grey(db, up, gmax, gmin)
        nwidth = int(np.float32(100.0) * np.float32(len(x)) / np.float32(sr))
        return np.asarray(O.grey_to_rgb(grey, nwidth, nh)[0], np.uint8)
    with ThreadPoolExecutor(min(16, len(pcm))) as ex:
        return list(ex.map(one, zip(pcm, srs, dbs)))


def _flipped(a, b):
    """Pixels of a that differ from b in any channel, and the largest channel difference."""
    d = np.abs(a.reshape(-1, 3).astype(np.int16) - b.reshape(-1, 3).astype(np.int16)).max(axis=1)
    return int((d > 0).sum()), int(d.max(initial=0))


def _check_multitrack(mt, pcm, srs, scale, nh, exact):
    """MultiTrack images against the oracle pipeline.

    exact (the reference-order kernel): the global range equals the oracle's and every image is
    the oracle pipeline's bytes.

    Otherwise SURVEY.md §8c as the reference's own f32 arithmetic allows it (round 5's diagnosis,
    scripts/diag_e2e_flips.py): a non-reference-order FFT differs from the oracle
    in bins 100+ dB below their frame's peak (f32 rounding noise: the 48 kHz substitute is 24 kHz
    content upsampled), where the oracle differs from the float64 spectrum as much (linear
    excerpts: oracle 1.15e-4, stft3 1.22e-4, stft5 1.41e-4 of the pixels against the float64
    image). Two consequences are held separately:
      range: the global max within 1e-3 dB of the oracle's; the global min -- the deepest value of
        the noise floor when the -120 dB clamp does not bind -- within max(DB_MAX, 2 x the
        oracle's own distance from the float64 min);
      images under the device's own range: at most 1 LSB anywhere, flipped pixels at most
        max(1e-4, 2 x the share the oracle's image flips against the float64 spectrum's image
        under that range)."""
    dbs, db64 = _oracle_specs(pcm, srs, scale, with_f64=not exact)
    ro = _global_range(dbs)
    rd = (mt.get_max_db(), mt.get_min_db())
    if exact:
        assert rd == ro, (rd, ro)
    else:
        r64 = _global_range(db64)
        assert abs(rd[0] - ro[0]) <= 1e-3, (rd, ro)
        assert abs(rd[1] - ro[1]) <= max(DB_MAX, 2 * abs(ro[1] - r64[1])), (rd, ro, r64)
        assert abs(rd[1] - ro[1]) <= E2E_GMIN_CAP_DB, (rd, ro)  # fixed cap beside the adaptive one
    ref = _oracle_images(pcm, srs, scale, nh, dbs, rd)
    f64 = None if exact else _oracle_images(pcm, srs, scale, nh, db64, rd)
    flips = f64_flips = total = worst = 0
    for i in range(len(pcm)):
        got = np.frombuffer(mt.get_spec_image(i, 100.0, nh), np.uint8)
        assert got.size == ref[i].size
        if exact:
            assert np.array_equal(got, ref[i].reshape(-1)), (i, _flipped(got, ref[i]))
            continue
        f, m = _flipped(got, ref[i])
        flips += f
        worst = max(worst, m)
        f64_flips += _flipped(ref[i], f64[i])[0]
        total += ref[i].size // 3
    if not exact:
        bound = max(E2E_MAX_FRAC, 2.0 * f64_flips / total)
        assert worst <= E2E_MAX_LSB and flips / total <= bound, (worst, flips, f64_flips, total)
        # a fixed cap beside the fixture-relative bound: a kernel regression cannot
        # hide behind a noisier fixture
        assert flips / total <= E2E_FLIP_CAP, (flips, total)
    return flips, f64_flips, total, dbs


@pytest.mark.parametrize("fast", [False, True])
@pytest.mark.parametrize("scale", [thesia.FreqScale.Mel, thesia.FreqScale.Linear])
def test_e2e_rgb_multitrack_samples(scale, fast):
    """MultiTrack (lib.rs:170-298) on the reference's sample excerpts + the 48 kHz substitute:
    get_spec_image bytes vs the oracle pipeline from the PCM -- equal bytes on the default
    (reference-order) path; fast = the streaming kernels at the viewer's geometries
    (thesia_mt_set_fast), held to _check_multitrack's contract."""
    z = np.load(fixtures.GOLDEN + "/samples_excerpt.npz")
    tags = ["8k", "16k", "22k05", "24k", "44k1"]
    pcm = [fixtures.s16_to_f32(z[f"pcm_{t}"]) for t in tags] + [fixtures.s16_to_f32(fixtures.c1_substitute()[:72000])]
    srs = [int(z[f"sr_{t}"]) for t in tags] + [48000]
    mt = thesia.MultiTrack(freq_scale=scale, fast=fast)
    mt.add_tracks_pcm(list(range(len(pcm))), pcm, srs)
    _check_multitrack(mt, pcm, srs, scale, 300, exact=not fast)
    mt.close()


@pytest.mark.parametrize("scale", [thesia.FreqScale.Mel, thesia.FreqScale.Linear])
def test_e2e_rgb_multitrack_fast_stft5(scale):
    """MultiTrack's fast path where it takes stft5: one add_tracks of 16
    48 kHz tracks x 250 s (25 000 frames each, 400 000 frames in the call's batch: the automatic
    rule's kView5MinFrames, engine.cpp), mel and linear rows, images vs the oracle pipeline under
    the same contract as the excerpts, plus the dB rows themselves."""
    from thesia import engine
    sr, n, k = 48000, 250 * 48000, 16
    pcm = [fixtures.s16_to_f32(engine.synth_pcm_host(1, i, n, sr, seed=5)).reshape(-1) for i in range(k)]
    win, hop, n_fft = O.track_params(sr)
    T = O.stft_n_frames(n, win, hop)
    assert k * T >= 400000
    # the automatic rule MultiTrack's fast path applies to this batch (auto_kernel, engine.cpp)
    kind = engine.OUT_MEL_AMP_DB if scale == thesia.FreqScale.Mel else engine.OUT_AMP_DB
    plan = engine.Plan(n_fft, win, hop, kind, sr=sr,
                       **({"mel_fb": O.calc_mel_fb_default(sr, n_fft)} if kind == engine.OUT_MEL_AMP_DB else {}))
    din, dout = engine.DeviceBuffer(8), engine.DeviceBuffer(8)
    b = engine.Batch(plan, din, [0] * k, [n] * k, dout)
    assert b.kernel == 5  # (never run: the buffers only stand in for the rule)
    b.close()
    plan.close()
    din.close()
    dout.close()
    mt = thesia.MultiTrack(freq_scale=scale, fast=True)
    mt.add_tracks_pcm(list(range(k)), pcm, [sr] * k)
    flips, f64_flips, total, dbs = _check_multitrack(mt, pcm, [sr] * k, scale, 300, exact=False)
    print(f"stft5 fast path: {flips} flipped of {total} px; the oracle vs float64: {f64_flips}")
    for i in (0, k - 1):
        mx, p = db_clamped_err(mt.get_spec(i), dbs[i])
        assert mx <= DB_MAX and p <= DB_P9999, (i, mx, p)
    mt.close()
