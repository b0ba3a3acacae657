"""Regenerate tests/golden/*.json from the oracle (CPU) on deterministic synthetic captures.

    python tests/golden/make_golden.py

Each fixture holds: the generator settings, SHA-256 of the capture bytes,
per-frame SHA-256 of the .tbc frame and .pcm audio, the per-frame metadata
(VBI + per-field records), and a few small per-stage vectors of the first
valid field read (demod channels around a sync pulse, final line locations).
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'ld-decode_amd'))

import numpy as np  # noqa: E402

from ldgpu.synth import NTSC, PAL, make_capture  # noqa: E402
from oracle.capture import FMT_BY_EXT, Capture  # noqa: E402
from oracle.comb import Comb2D  # noqa: E402
from oracle.demod import RFDemod  # noqa: E402
from oracle.field import FieldNTSC, FieldPAL  # noqa: E402
from oracle.framer import decode_capture  # noqa: E402

CASES = {
    'ntsc_cav_u8_0p2s': dict(seconds=0.2, fmt='u8', system='NTSC', kw={}),
    'ntsc_clv_u8_0p2s': dict(seconds=0.2, fmt='u8', system='NTSC', kw={'clv': True, 'first_frame': 5399}),
    'ntsc_cav_r30_0p15s': dict(seconds=0.15, fmt='r30', system='NTSC', kw={'seed': 7}),
    'ntsc_cav_lds_0p15s': dict(seconds=0.15, fmt='lds', system='NTSC', kw={'seed': 8}),
    'pal_clv_u8_0p2s': dict(seconds=0.2, fmt='u8', system='PAL',
                            kw={'clv': True, 'first_frame': 3000, 'seed': 5}),
    # the s16 loader (lddutils.py:131-147)
    'ntsc_cav_s16_0p15s': dict(seconds=0.15, fmt='s16', system='NTSC', kw={'seed': 9}),
    # a capture that starts 300,000 samples into a field (the first read's short
    # nextfieldoffset, demod's start-1024 quirk at the file start, lddecode_core.py:378-380)
    'ntsc_cav_u8_mid_0p2s': dict(seconds=0.2, fmt='u8', system='NTSC', kw={'seed': 10}, skip=300000),
    # the MTF chain away from MTF ~ 1 (Framer.readframe, lddecode_core.py:1300-1309; demodblock
    # :292-293): a CAV capture from picture ~1200, whose first frame is decoded at MTF 1, then
    # dropped and the next one re-read at MTF 0.88 ...
    'ntsc_cav_u8_mtf_0p3s': dict(seconds=0.3, fmt='u8', system='NTSC', kw={'seed': 11, 'first_frame': 1200}),
    # ... one crossing picture 9999 -> 10001, where the MTF clamps to 0 and demodblock skips
    # the MTF product (mtf_level == 0) ...
    'ntsc_cav_u8_mtf0_0p3s': dict(seconds=0.3, fmt='u8', system='NTSC', kw={'seed': 12, 'first_frame': 9997}),
    # ... and a PAL CAV disc from picture ~1200 (the same chain on FieldPAL)
    'pal_cav_u8_mtf_0p3s': dict(seconds=0.3, fmt='u8', system='PAL', kw={'seed': 13, 'first_frame': 1200}),
    # PAL through the 10-bit loaders (the demod's .lds / .r30 unpacking with PAL's geometry)
    'pal_clv_lds_0p15s': dict(seconds=0.15, fmt='lds', system='PAL', kw={'clv': True, 'first_frame': 3000, 'seed': 14}),
    'pal_cav_r30_0p15s': dict(seconds=0.15, fmt='r30', system='PAL', kw={'seed': 15}),
}


def wow(system, amp1, amp2, phase2=1.1):
    """Two disc-speed components (SynthRF's ``wow``): a flutter of 37.3 lines' period and a
    wow of 1.7 fields' period, so that no two lines or fields of a capture see the same error."""
    spl = 40e6 * (NTSC if system == 'NTSC' else PAL)['line_us'] / 1e6
    field_lines = 262.5 if system == 'NTSC' else 312.5
    return ((amp1, 37.3 * spl, 0.4), (amp2, 1.7 * field_lines * spl, phase2))


# captures with time-base error: every capture above comes from a rigid clock (line spans
# 2542 +- 1 / 2560 +- 1 samples), which leaves the time-base corrector at its fixed point
CASES.update({
    # line spans ~ +-9 samples around nominal, nextfieldoffset hundreds of samples off the clean chain
    'ntsc_cav_u8_wow_0p2s': dict(seconds=0.2, fmt='u8', system='NTSC',
                                 kw={'seed': 31, 'wow': wow('NTSC', 0.0015, 0.002)}),
    # line spans ~ +-25 samples: gaps outside linelen +- 0.2 us, so refine_linelocs_hsync's head /
    # tail repair replaces them (lddecode_core.py:767-785); frames off nominal by more than the
    # planner's probe half-window (762 samples; with the wow at the other cases' phase 1.1 the
    # three frame lengths of 0.2 s stay within 728 of nominal, at 0.35 the first is ~790 short)
    'ntsc_cav_u8_wowbig_0p2s': dict(seconds=0.2, fmt='u8', system='NTSC',
                                    kw={'seed': 31, 'wow': wow('NTSC', 0.006, 0.004, phase2=0.35)}),
    'pal_clv_u8_wow_0p25s': dict(seconds=0.25, fmt='u8', system='PAL',
                                 kw={'clv': True, 'first_frame': 3000, 'seed': 31,
                                     'wow': wow('PAL', 0.0015, 0.002)}),
    'pal_cav_u8_wowbig_0p25s': dict(seconds=0.25, fmt='u8', system='PAL',
                                    kw={'seed': 31, 'wow': wow('PAL', 0.006, 0.004)}),
    # frame lengths a few to tens of samples off nominal: inside the probe window, outside the
    # planner's exact prediction
    'ntsc_cav_u8_jit_0p3s': dict(seconds=0.3, fmt='u8', system='NTSC',
                                 kw={'seed': 31, 'wow': wow('NTSC', 0.00002, 0.0001)}),
    'pal_clv_u8_jit_0p3s': dict(seconds=0.3, fmt='u8', system='PAL',
                                kw={'clv': True, 'first_frame': 3000, 'seed': 31,
                                    'wow': wow('PAL', 0.00002, 0.0001)}),
    # the same timing behind the 10-bit .lds packing groups
    'ntsc_cav_lds_wow_0p15s': dict(seconds=0.15, fmt='lds', system='NTSC',
                                   kw={'seed': 31, 'wow': wow('NTSC', 0.0015, 0.002)}),
})


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def build_capture(case):
    c = CASES[case]
    skip = c.get('skip', 0)
    data = make_capture(int(40e6 * c['seconds']) + skip, c['fmt'], system=c['system'], **c['kw'])
    if skip:
        assert c['fmt'] in ('u8', 's16')
        data = data[skip * (2 if c['fmt'] == 's16' else 1):]
    return data


def make(case):
    c = CASES[case]
    data = build_capture(case)
    fmt = FMT_BY_EXT[c['fmt']]
    frames, pcm, meta = decode_capture(data, fmt, system=c['system'])
    out = {'case': case, 'settings': {k: v for k, v in c.items()}, 'capture_sha256': sha(data),
           'frames': [{'tbc_sha256': sha(f.tobytes()), 'pcm_sha256': sha(a.tobytes()), 'pcm_len': int(a.size),
                       'meta': m} for f, a, m in zip(frames, pcm, meta)]}
    if c['system'] == 'NTSC' and frames:
        # the frames through the 2D comb restatement (one comb process, in order)
        rgb = Comb2D().process(np.stack(frames))
        for g, r in zip(out['frames'], rgb):
            g['comb_rgb48_sha256'] = sha(r.tobytes())
    # per-stage vectors of the first valid field
    rf = RFDemod(system=c['system'])
    cap = Capture(data, fmt)
    first = next(fr for m in meta for fr in m['fields'] if fr['valid'])
    raw = rf.demod(cap, first['readsample'], 1000000, first['mtf_level'])
    f = (FieldNTSC if c['system'] == 'NTSC' else FieldPAL)(rf, raw, 0, audio_offset=0)
    p = int(f.peaklist[20])
    out['stage'] = {'readsample': first['readsample'], 'mtf_level': first['mtf_level'], 'peak20': p,
                    'demod': raw[0]['demod'][p - 8:p + 8].tolist(),
                    'demod_05': raw[0]['demod_05'][p - 8:p + 8].tolist(),
                    'demod_sync': raw[0]['demod_sync'][p - 8:p + 8].tolist(),
                    'demod_burst': raw[0]['demod_burst'][p - 8:p + 8].tolist(),
                    'linelocs': [float(x) for x in f.linelocs[:12]],
                    'burstlevel': [float(x) for x in getattr(f, 'burstlevel', [])[:12]]}
    path = os.path.join(HERE, case + '.json')
    with open(path, 'w') as fh:
        json.dump(out, fh, indent=1)
    print('wrote', path, len(frames), 'frames')


if __name__ == '__main__':
    for case in (sys.argv[1:] or CASES):
        make(case)
