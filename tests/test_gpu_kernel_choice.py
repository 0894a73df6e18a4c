"""Characterisation of the batch kernel selection rule (engine.cpp: the selection table,
auto_kernel, THESIA_BATCH_OPT_KERNEL) against tests/golden/kernel_choice.json, recorded from the
library before the rule was gathered into one table.

Per case (geometry, input format, channels, output kind, frame count) the fixture holds
  [automatic kernel, automatic kernel with OPT_RANGE set (null for complex rows),
   the ids of 1, 2, 3, 5, 7, 9 that OPT_KERNEL accepts (the others raise ERR_UNSUPPORTED)].
Nothing is launched: input and output are 8-byte stand-in buffers, and the range pointer is
never written."""
import json
import os

import pytest

from thesia import engine
from thesia._lib import ERR_UNSUPPORTED, ThesiaError

pytestmark = pytest.mark.gpu

KERNEL_IDS = (1, 2, 3, 5, 7, 9)
KINDS = {"complex": engine.OUT_COMPLEX, "amp_db": engine.OUT_AMP_DB, "power_db": engine.OUT_POWER_DB,
         "mel_amp_db": engine.OUT_MEL_AMP_DB}
FORMATS = {"f32": engine.IN_F32, "s16": engine.IN_S16}
CHANNELS = (1, 2, 3)
VIEW5_MIN_FRAMES = 400_000  # the automatic rule's threshold at the 48 kHz viewer geometry

# (win, hop, n_fft, sr): canonical; the viewer's geometries (oracle_ffi.track_params of the sr);
# an odd win; a hop that no streaming kernel takes
GEOMETRIES = ([(n, n // 4, n, 48000) for n in (128, 256, 512, 1024, 2048, 4096)] +
              [(320, 80, 512, 8000), (640, 160, 1024, 16000), (960, 240, 1024, 24000),
               (1920, 480, 2048, 48000), (1764, 441, 2048, 44100), (884, 221, 1024, 22050)] +
              [(1001, 250, 1024, 48000), (1024, 300, 1024, 48000)])


def _geo_id(g):
    return "%d-%d-%d" % g[:3]


def _variants(geo):
    """(kind name, n_mels, frames name, track length) of a geometry: every kind with the 128-mel
    bank on a short track; a 512-mel bank at n_fft 2048 (the LDS-fit terms of the rule see
    their largest mel tables; the recorded rule still accepts every kernel there); at the 48 kHz viewer geometry, tracks just below and at the automatic rule's threshold."""
    win, hop, n_fft, _ = geo
    short = 5 * n_fft + 7
    out = [(k, 128 if k == "mel_amp_db" else 0, "short", short) for k in KINDS]
    if n_fft == 2048:
        out.append(("mel_amp_db", 512, "short", short))
    if (win, hop, n_fft) == (1920, 480, 2048):
        for k in KINDS:
            n_mels = 128 if k == "mel_amp_db" else 0
            out.append((k, n_mels, "below", (VIEW5_MIN_FRAMES - 2) * hop))
            out.append((k, n_mels, "at", (VIEW5_MIN_FRAMES - 1) * hop))
    return out


def observe(geo):
    """{case id: [auto, auto with the range option, accepted ids]} of one geometry."""
    win, hop, n_fft, sr = geo
    din, dout, drange = engine.DeviceBuffer(8), engine.DeviceBuffer(8), engine.DeviceBuffer(12)
    got = {}
    plans = {}
    for kind, n_mels, frames, n in _variants(geo):
        if (kind, n_mels) not in plans:
            plans[kind, n_mels] = engine.Plan(n_fft, win, hop, KINDS[kind], sr=sr, n_mels=n_mels)
        plan = plans[kind, n_mels]
        total = engine.Batch.frames_for(plan, [n])
        if frames != "short":
            assert total == VIEW5_MIN_FRAMES - (frames == "below"), (frames, total)
        for fmt, inf in FORMATS.items():
            for ch in CHANNELS:
                b = engine.Batch(plan, din, [0], [n], dout, input_format=inf, channels=ch)
                auto = b.kernel
                accepted = []
                for k in KERNEL_IDS:
                    try:
                        b.set_option(engine.OPT_KERNEL, k)
                    except ThesiaError as e:
                        assert e.code == ERR_UNSUPPORTED, (k, e)
                        continue
                    assert b.kernel == k
                    accepted.append(k)
                b.set_option(engine.OPT_KERNEL, 0)
                assert b.kernel == auto
                auto_range = None
                if kind != "complex":
                    b.set_option(engine.OPT_RANGE, drange.ptr.value)
                    auto_range = b.kernel
                b.close()
                case = "%s/%s/%dch/%s%s/%s" % (_geo_id(geo), fmt, ch, kind, n_mels or "", frames)
                got[case] = [auto, auto_range, accepted]
    for p in plans.values():
        p.close()
    for buf in (din, dout, drange):
        buf.close()
    return got


@pytest.fixture(scope="module")
def recorded(golden_dir):
    with open(os.path.join(golden_dir, "kernel_choice.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("geo", GEOMETRIES, ids=_geo_id)
def test_kernel_choice_equals_the_recorded_rule(geo, recorded):
    got = observe(geo)
    want = {c: v for c, v in recorded.items() if c.startswith(_geo_id(geo) + "/")}
    assert got.keys() == want.keys()
    diff = {c: (got[c], want[c]) for c in got if got[c] != want[c]}
    assert not diff, diff


def test_fixture_holds_no_other_cases(recorded):
    ids = {_geo_id(g) for g in GEOMETRIES}
    assert {c.split("/")[0] for c in recorded} == ids
