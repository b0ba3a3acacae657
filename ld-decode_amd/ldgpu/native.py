"""ctypes binding of libldgpu.so (include/ldgpu.h).

The library is built in-tree (``ld-decode_amd/ldgpu/libldgpu.so``) by
``__graft_entry__.build()``.  There is no CPU fallback: if the library or a
GPU is missing, ``load()`` / ``Context`` raise.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, 'libldgpu.so')

LDG_OK = 0
FS_VALID, FS_NO_VSYNC, FS_SHORT, FS_LINELOCS, FS_TBC, FS_EOF, FS_CRASH, FS_PENDING, FS_MIGRATED, FS_VCUT = range(10)
VBI_NONE = -2147483648
READ_FULL, READ_PROBE = 1, 2            # ldg_decode_reads_async2 per-read flags (include/ldgpu.h)
LOG_NO_VSYNC = 1 << 16            # ldg_field_info.log_flags (include/ldgpu.h)
MAX_VSYNCS = 16

EXPORTS = ['ldg_create', 'ldg_destroy', 'ldg_last_error', 'ldg_set_filters', 'ldg_set_capture',
           'ldg_decode_reads', 'ldg_field_audio', 'ldg_assemble_frames', 'ldg_debug_read',
           'ldg_comb_ntsc', 'ldg_comb_reset', 'ldg_version', 'ldg_device_count', 'ldg_profile_enable',
           'ldg_profile_read', 'ldg_synth_capture', 'ldg_capture_download', 'ldg_comb_ntsc_async', 'ldg_sync', 'ldg_demod_isolated', 'ldg_demod_isolated_ex', 'ldg_comb_set_opts', 'ldg_output_async', 'ldg_output_wait',
           'ldg_host_alloc', 'ldg_host_free',
           'ldg_archive_fields', 'ldg_archive_audio', 'ldg_decode_reads_async', 'ldg_decode_reads_async2',
           'ldg_set_video_cut', 'ldg_tail_plan', 'ldg_audio_reach', 'ldg_div_const', 'ldg_decode_reads_wait',
           'ldg_field_audio_async', 'ldg_field_audio_collect', 'ldg_comb_ntsc3d', 'ldg_cx_create', 'ldg_cx_destroy', 'ldg_cx_process', 'ldg_comb_pal', 'ldg_comb_set_state', 'ldg_profile_spans', 'ldg_profile_spans_union', 'ldg_profile_span_table',
           'ldg_audio_offsets', 'ldg_comb_async', 'ldg_debug_rf_table',
           'ldg_stream_open', 'ldg_stream_release', 'ldg_stream_seek', 'ldg_stream_window', 'ldg_stream_stats',
           'ldg_stream_close', 'ldg_device_memory',
           'ldg_dropout_defaults', 'ldg_set_dropout_opts', 'ldg_field_dropouts',
           'ldg_stack_frames', 'ldg_conceal_frames', 'ldg_stack_stats',
           'ldg_efm_defaults', 'ldg_efm_set_opts', 'ldg_efm_window', 'ldg_efm_extract', 'ldg_efm_debug_read',
           'ldg_efmdec_set_table', 'ldg_efmdec_reset', 'ldg_efmdec_feed', 'ldg_efmdec_read',
           'ldg_efmsec_enable', 'ldg_efmsec_reset', 'ldg_efmsec_feed', 'ldg_efmsec_last_info', 'ldg_efmsec_read',
           'ldg_field_line_services', 'ldg_frames_line_services',
           'ldg_flac_open', 'ldg_flac_index', 'ldg_flac_frames', 'ldg_flac_read', 'ldg_flac_capture', 'ldg_flac_close']
STACK_MAX_SOURCES = 16            # LDG_STACK_MAX_SOURCES
STACK_MODES = {'median': 0, 'mean': 1, 'smart-mean': 2}      # LDG_STACK_*
STACK_STATS = ('h2d_s', 'kernel_s', 'd2h_s', 'calls')        # ldg_stack_stats, in order
FRAME_SHAPE = {'NTSC': (525, 910), 'PAL': (625, 1135)}       # .tbc frame rows, pixels
MAX_DROPOUTS_PER_LINE = 8         # LDG_MAX_DROPOUTS_PER_LINE
MAX_LINES = 320                   # rows of the per-slot line arrays (ldg_debug_read)
STREAM_STATS = ('bytes_read', 'read_s', 'chunks', 'launch_waits', 'launch_wait_s', 'space_wait_s', 'seeks',
                'ring_bytes', 'chunk_bytes', 'stage_wait_s')     # ldg_stream_stats, in order


class FieldInfo(C.Structure):
    _fields_ = [('status', C.c_int32), ('npeaks', C.c_int32), ('nvsync', C.c_int32), ('istop', C.c_int32),
                ('linecount', C.c_int32), ('nlines', C.c_int32), ('n_out', C.c_int64),
                ('nextfieldoffset', C.c_int64), ('tbcstart', C.c_int64), ('med_hsync', C.c_double),
                ('hsync_tol', C.c_double), ('vsync', (C.c_int32 * 3) * MAX_VSYNCS),
                ('linecode', (C.c_int32 * 6) * 3), ('linecode_ok', C.c_int32 * 3),
                ('vbi_minutes', C.c_int32), ('vbi_seconds', C.c_int32), ('vbi_clvframe', C.c_int32),
                ('vbi_framenr', C.c_int32), ('vbi_status', C.c_int32), ('vbi_isclv', C.c_int32),
                ('burst_group', C.c_int32), ('log_flags', C.c_int32), ('pad_', C.c_int32),
                ('readsample', C.c_int64)]


class Config(C.Structure):
    _fields_ = [('system', C.c_int32), ('device', C.c_int32), ('max_reads', C.c_int32),
                ('max_frames', C.c_int32)]


class Params(C.Structure):
    _fields_ = [('freq_hz', C.c_double), ('freq', C.c_double), ('ire0', C.c_double), ('hz_ire', C.c_double),
                ('vsync_ire', C.c_double), ('sync_lo', C.c_double), ('sync_hi', C.c_double),
                ('freq_arf', C.c_double), ('audio_lowfreq', C.c_double), ('audio_lfreq', C.c_double),
                ('audio_rfreq', C.c_double), ('line_period', C.c_double), ('fsc_mhz', C.c_double),
                ('linelen', C.c_int32), ('outlinelen', C.c_int32), ('frame_lines', C.c_int32),
                ('audio_lo0', C.c_int32), ('codelines', C.c_int32 * 3), ('pad_', C.c_int32)]


class KernelStat(C.Structure):
    _fields_ = [('name', C.c_char * 48), ('launches', C.c_int64), ('total_ms', C.c_double)]


class SynthParams(C.Structure):
    _fields_ = [('fmt', C.c_int32), ('pad_', C.c_int32), ('nsamples', C.c_int64), ('seed', C.c_uint64),
                ('noise', C.c_double), ('start_line', C.c_double)]


_DP = C.POINTER(C.c_double)


class CombOpts(C.Structure):
    """ldg_comb_opts (include/ldgpu.h): comb-ntsc's command-line options."""
    _fields_ = [('black_ire', C.c_double), ('brightness', C.c_double), ('nr_y', C.c_double), ('nr_c', C.c_double),
                ('bw', C.c_int32), ('adaptive2d', C.c_int32), ('colorlpf', C.c_int32), ('colorlpf_hq', C.c_int32),
                ('linesout', C.c_int32), ('debug_line', C.c_int32), ('wide', C.c_int32),
                ('opticalflow', C.c_int32)]


class DropoutOpts(C.Structure):
    """ldg_dropout_opts (include/ldgpu.h): the build-defined dropout detector's options."""
    _fields_ = [('lo_ire', C.c_double), ('hi_ire', C.c_double), ('merge_gap', C.c_int32),
                ('min_flagged', C.c_int32), ('pad', C.c_int32), ('conceal', C.c_int32)]


class Dropout(C.Structure):
    """ldg_dropout: pixels [startx, endx) of field row `row`."""
    _fields_ = [('row', C.c_int16), ('startx', C.c_int16), ('endx', C.c_int16), ('pad_', C.c_int16)]


class LineServices(C.Structure):
    """ldg_line_services: the white flag, closed captions and video ID of one NTSC field."""
    _fields_ = [('white_count', C.c_int32), ('white_flag', C.c_int32), ('cc_state', C.c_int32),
                ('cc_runin', C.c_int32), ('cc_x', C.c_int32), ('cc', C.c_uint8 * 2), ('pad_', C.c_uint8 * 2),
                ('vid_state', C.c_int32), ('vid_x', C.c_int32), ('vid_bits', C.c_int32)]


LINE_SERVICES_SIZE = 36           # LDG_LINE_SERVICES_SIZE
LINE_ABSENT, LINE_OK, LINE_CHECK, LINE_FRAME = range(4)      # LDG_LINE_*


def line_records(arr):
    """The ldg_line_services of a numpy view (any shape) as a flat list of dicts of their members."""
    return [{'white_count': wc, 'white_flag': wf, 'cc_state': cs, 'cc_runin': cr, 'cc_x': cx,
             'cc': (int(cc[0]), int(cc[1])), 'vid_state': vs, 'vid_x': vx, 'vid_bits': vb}
            for wc, wf, cs, cr, cx, cc, _, vs, vx, vb in arr.reshape(-1).tolist()]


def line_services_json(d):
    """One of line_records as the 'lineServices' of a field's metadata: the caption bytes where a start
    bit was found, the 14 data bits of the video ID where its CRC holds."""
    return {'white': bool(d['white_flag']), 'whiteCount': d['white_count'],
            'cc': [d['cc'][0], d['cc'][1]] if d['cc_state'] != LINE_ABSENT else None, 'ccState': d['cc_state'],
            'videoId': d['vid_bits'] >> 6 if d['vid_state'] == LINE_OK else None,
            'videoIdBits': d['vid_bits'], 'videoIdState': d['vid_state']}


class FlacInfo(C.Structure):
    """ldg_flac_info: the container and STREAMINFO of an open FLAC-compressed capture."""
    _fields_ = [('container', C.c_int32), ('fmt', C.c_int32), ('bps', C.c_int32), ('channels', C.c_int32),
                ('sample_rate', C.c_int32), ('min_block', C.c_int32), ('max_block', C.c_int32), ('pad_', C.c_int32),
                ('total_samples', C.c_int64), ('file_bytes', C.c_int64), ('audio_offset', C.c_int64),
                ('md5', C.c_uint8 * 16)]


FLAC_COUNTERS = ('candidates', 'header_ok', 'parsed', 'accepted', 'kept', 'nested', 'misplaced', 'range',
                 'ogg_broken', 'lost_bytes', 'gaps', 'gap_samples')


class FlacCounters(C.Structure):
    """ldg_flac_counters: what ldg_flac_index found."""
    _fields_ = [(k, C.c_int64) for k in FLAC_COUNTERS + ('nsamples', 'frames')]


# ldg_flac_frame
FLAC_FRAME = np.dtype([('offset', '<i8'), ('bytes', '<i8'), ('position', '<i8'), ('block_size', '<i4'),
                       ('state', '<i4')])
FLAC_INFO_SIZE, FLAC_COUNTERS_SIZE, FLAC_FRAME_SIZE = 72, 112, 32      # LDG_FLAC_*_SIZE
FLAC_KEPT, FLAC_NESTED, FLAC_MISPLACED = range(3)                      # LDG_FLAC_*


class EfmOpts(C.Structure):
    """ldg_efm_opts (include/ldgpu.h): the build-defined EFM run-length extraction's options."""
    _fields_ = [('fs', C.c_double), ('alpha', C.c_double), ('beta', C.c_double), ('delta', C.c_double),
                ('keep_debug', C.c_int32), ('pad_', C.c_int32)]


class EfmSeg(C.Structure):
    """ldg_efm_seg: one segment's counters."""
    _fields_ = [('emitted', C.c_int64), ('ignored', C.c_int64), ('clamped_low', C.c_int64),
                ('clamped_high', C.c_int64), ('final_P', C.c_double)]


class EfmdecInfo(C.Structure):
    """ldg_efmdec_info: what one ldg_efmdec_feed added, and its counters."""
    _fields_ = [(k, C.c_int64) for k in (
        'first_frame', 'frames', 'first_sample', 'samples', 'candidates', 'confirmed', 'coasted', 'breaks',
        'bad_symbols', 'c1_pass', 'c1_fixed', 'c1_erased', 'c2_pass', 'c2_fixed', 'c2_erasure_solved', 'c2_failed',
        'c2_unsolved', 'flagged', 'averaged', 'muted', 'held_runs')]


# ldg_efmdec_read: name -> (LDG_EFMDEC_*, dtype, values per sample or frame)
EFMDEC_ARRAYS = {'pcm': (0, np.int16, 2), 'flags': (1, np.uint8, 2), 'subcode': (2, np.uint16, 1),
                 'starts': (10, np.int64, 1), 'f3': (11, np.uint8, 32), 'c1': (12, np.uint8, 28),
                 'c1_flags': (13, np.uint8, 1), 'c2': (14, np.uint8, 28), 'c2_flags': (15, np.uint32, 1)}

class EfmsecInfo(C.Structure):
    """ldg_efmsec_info: what one call of the data-sector stage added, and its counters."""
    _fields_ = [(k, C.c_int64) for k in (
        'first_byte', 'bytes', 'first_sector', 'sectors', 'candidates', 'confirmed', 'coasted', 'breaks', 'good',
        'corrected', 'bad', 'other', 'p_fixed', 'q_fixed', 'erased_bytes', 'held_bytes')]


# ldg_efmsec_rec: a sector's status (LDG_EFMSEC_*), rounds, erased bytes and header as stored
EFMSEC_REC = np.dtype([('status', '<i4'), ('rounds', '<i4'), ('erased', '<i4'), ('minute', 'u1'), ('second', 'u1'),
                       ('frame', 'u1'), ('mode', 'u1')])
# ldg_efmsec_read: name -> (LDG_EFMSEC_*, dtype, values per sector or byte)
EFMSEC_ARRAYS = {'data': (0, np.uint8, 2048), 'sectors': (1, np.uint8, 2352), 'records': (2, EFMSEC_REC, 1),
                 'starts': (3, np.int64, 1), 'bytes': (10, np.uint8, 1), 'erased': (11, np.uint8, 1)}

EFM_SEG = 1 << 20                 # RF samples per EFM segment (csrc/efm_plan.hpp SEG)
EFM_NTAPS = 255
EFM_CHANNEL_HZ = 4321800.0


def efm_defaults():
    """ldg_efm_defaults as a dict (keys of ldg_efm_opts); no device needed."""
    o = EfmOpts()
    if load().ldg_efm_defaults(C.byref(o)) != LDG_OK:
        raise LDGError('ldg_efm_defaults failed')
    return {k: getattr(o, k) for k, _ in EfmOpts._fields_ if k != 'pad_'}


def efm_window(seg_lo, seg_hi, file_nsamples):
    """ldg_efm_window: the samples [lo, hi) of the file that segments [seg_lo, seg_hi) read
    ((0, 0): none).  Host code, no device needed."""
    out = np.zeros(2, dtype=np.int64)
    if load().ldg_efm_window(int(seg_lo), int(seg_hi), int(file_nsamples), out.ctypes.data) != LDG_OK:
        raise ValueError('ldg_efm_window: invalid segment range (%r, %r, %r)' % (seg_lo, seg_hi, file_nsamples))
    return int(out[0]), int(out[1])


def dropout_defaults(system):
    """ldg_dropout_defaults as a dict (keys of ldg_dropout_opts); no device needed."""
    o = DropoutOpts()
    if load().ldg_dropout_defaults(1 if system == 'PAL' else 0, C.byref(o)) != LDG_OK:
        raise LDGError('ldg_dropout_defaults failed')
    return {k: getattr(o, k) for k, _ in DropoutOpts._fields_}


COMB_DEFAULTS = dict(black_ire=7.5, brightness=236.0, nr_y=1.0, nr_c=0.0, bw=False, adaptive2d=True, colorlpf=True,
                     colorlpf_hq=True, linesout=480, debug_line=-1000, wide=False, opticalflow=False)


class Filters(C.Structure):
    _fields_ = [(k, _DP) for k in ('rfvideo', 'mtf', 'fvideo', 'fvideo05', 'fvideoburst', 'fvideopilot', 'fpsync',
                                   'audio_lfilt', 'audio_rfilt', 'audio_lpf2', 'mtf_logabs', 'mtf_arg', 'iir',
                                   'f05_fir')]


_lib = None


def lib_source_hash():
    """The source hash (build.py source_hash) of the loaded libldgpu.so: its build stamp, or
    None when the library carries none (a variant build loaded through LDGPU_LIB)."""
    lib = load()
    stamp = lib._name + '.sha256'
    return open(stamp).read().strip() if os.path.exists(stamp) else None


def load(path=None):
    """Load libldgpu.so and declare its signatures (no device access).
    LDGPU_LIB names another build of the same library (profiling variants)."""
    global _lib
    if _lib is not None:
        return _lib
    path = path or os.environ.get('LDGPU_LIB') or LIB_PATH
    if not os.path.exists(path):
        raise RuntimeError('libldgpu.so not built (%s); run __graft_entry__.build()' % path)
    lib = C.CDLL(path)
    vp = C.c_void_p
    lib.ldg_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    lib.ldg_destroy.argtypes = [vp]
    lib.ldg_last_error.argtypes = [vp]
    lib.ldg_last_error.restype = C.c_char_p
    lib.ldg_set_filters.argtypes = [vp, C.POINTER(Params), C.POINTER(Filters)]
    lib.ldg_set_capture.argtypes = [vp, vp, C.c_int64, C.c_int, C.c_int64, C.c_int]
    lib.ldg_decode_reads.argtypes = [vp, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_double),
                                     C.POINTER(C.c_int32), C.POINTER(FieldInfo)]
    lib.ldg_field_audio.argtypes = [vp, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_double),
                                    C.POINTER(C.c_int16), C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_double)]
    lib.ldg_field_audio_async.argtypes = [vp, C.c_int, vp, vp]
    lib.ldg_field_audio_collect.argtypes = [vp, vp, C.c_int64, vp, vp]
    lib.ldg_assemble_frames.argtypes = [vp, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                        C.POINTER(C.c_uint16), C.c_int]
    lib.ldg_debug_read.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int64]
    lib.ldg_debug_read.restype = C.c_int64
    lib.ldg_debug_rf_table.argtypes = [vp, C.c_double, vp]
    lib.ldg_comb_ntsc.argtypes = [vp, C.c_int, vp, vp, C.c_int]
    lib.ldg_comb_reset.argtypes = [vp]
    lib.ldg_comb_set_opts.argtypes = [vp, C.POINTER(CombOpts)]
    lib.ldg_output_async.argtypes = [vp, C.c_int, vp, vp, vp, vp]
    lib.ldg_output_wait.argtypes = [vp]
    lib.ldg_host_alloc.argtypes = [C.c_int64, C.POINTER(vp)]
    lib.ldg_host_free.argtypes = [vp]
    lib.ldg_comb_ntsc_async.argtypes = [vp, C.c_int]
    lib.ldg_comb_async.argtypes = [vp, C.c_int]
    lib.ldg_comb_ntsc3d.argtypes = [vp, C.c_int, vp, vp, C.POINTER(C.c_int), C.c_double, C.c_double]
    lib.ldg_decode_reads_async.argtypes = [vp, C.c_int, vp, vp, vp]
    lib.ldg_decode_reads_async2.argtypes = [vp, C.c_int, vp, vp, vp, vp]
    lib.ldg_set_video_cut.argtypes = [vp, C.c_int64]
    lib.ldg_tail_plan.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_int64, vp]
    lib.ldg_div_const.argtypes = [vp, C.c_int64, C.c_double, C.c_int, vp]
    lib.ldg_audio_reach.argtypes = [vp, C.c_int, C.c_int, C.c_double, vp]
    lib.ldg_decode_reads_wait.argtypes = [vp, vp]
    lib.ldg_archive_fields.argtypes = [vp, C.c_int, vp, C.c_int64]
    lib.ldg_archive_audio.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int64, vp, vp]
    lib.ldg_sync.argtypes = [vp]
    lib.ldg_demod_isolated.argtypes = [vp, C.c_int, vp, C.c_int, C.POINTER(C.c_double)]
    lib.ldg_demod_isolated_ex.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.POINTER(C.c_double)]
    lib.ldg_profile_enable.argtypes = [vp, C.c_int]
    lib.ldg_profile_read.argtypes = [vp, C.POINTER(KernelStat), C.c_int]
    lib.ldg_profile_spans.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    lib.ldg_profile_spans_union.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    lib.ldg_profile_span_table.argtypes = [vp, vp, C.c_int]
    lib.ldg_synth_capture.argtypes = [vp, C.POINTER(SynthParams), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                      C.POINTER(C.c_uint32), C.c_int64]
    lib.ldg_capture_download.argtypes = [vp, vp, C.c_int64, C.c_int64]
    lib.ldg_capture_download.restype = C.c_int64
    lib.ldg_comb_pal.argtypes = [vp, C.c_int, vp, vp]
    lib.ldg_comb_set_state.argtypes = [vp, C.c_double]
    lib.ldg_cx_create.argtypes = [C.POINTER(vp)]
    lib.ldg_cx_destroy.argtypes = [vp]
    lib.ldg_cx_process.argtypes = [vp, C.c_int64, vp, vp]
    lib.ldg_audio_offsets.argtypes = [C.c_double, C.c_int64, vp, C.c_double, vp]
    lib.ldg_stream_open.argtypes = [vp, C.c_char_p, C.c_int, C.c_int64, C.c_int64]
    lib.ldg_stream_release.argtypes = [vp, C.c_int64]
    lib.ldg_stream_seek.argtypes = [vp, C.c_int64]
    lib.ldg_stream_window.argtypes = [vp, vp]
    lib.ldg_stream_stats.argtypes = [vp, vp, C.c_int]
    lib.ldg_stream_close.argtypes = [vp]
    lib.ldg_device_memory.argtypes = [C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.ldg_dropout_defaults.argtypes = [C.c_int, C.POINTER(DropoutOpts)]
    lib.ldg_set_dropout_opts.argtypes = [vp, C.POINTER(DropoutOpts)]
    lib.ldg_field_dropouts.argtypes = [vp, C.c_int, vp, vp, C.c_int64, vp]
    lib.ldg_stack_frames.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, C.c_int, vp]
    lib.ldg_conceal_frames.argtypes = [vp, C.c_int, vp, vp, vp, vp]
    lib.ldg_stack_stats.argtypes = [vp, vp, C.c_int]
    lib.ldg_efm_defaults.argtypes = [C.POINTER(EfmOpts)]
    lib.ldg_efm_set_opts.argtypes = [vp, C.POINTER(EfmOpts), vp, C.c_int]
    lib.ldg_efm_window.argtypes = [C.c_int64, C.c_int64, C.c_int64, vp]
    lib.ldg_efm_extract.argtypes = [vp, vp, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int64, vp,
                                    C.c_int64, C.POINTER(C.c_int64), vp]
    lib.ldg_efm_debug_read.argtypes = [vp, C.c_int, vp, C.c_int64, C.POINTER(C.c_int64)]
    lib.ldg_efm_debug_read.restype = C.c_int64
    lib.ldg_efmdec_set_table.argtypes = [vp, vp, C.c_int]
    lib.ldg_efmdec_reset.argtypes = [vp]
    lib.ldg_efmdec_feed.argtypes = [vp, vp, C.c_int64, C.c_int, C.POINTER(EfmdecInfo)]
    lib.ldg_efmdec_read.argtypes = [vp, C.c_int, vp, C.c_int64, C.POINTER(C.c_int64)]
    lib.ldg_efmdec_read.restype = C.c_int64
    lib.ldg_efmsec_enable.argtypes = [vp, C.c_int]
    lib.ldg_efmsec_reset.argtypes = [vp]
    lib.ldg_efmsec_feed.argtypes = [vp, vp, vp, C.c_int64, C.c_int, C.POINTER(EfmsecInfo)]
    lib.ldg_efmsec_last_info.argtypes = [vp, C.POINTER(EfmsecInfo)]
    lib.ldg_efmsec_read.argtypes = [vp, C.c_int, vp, C.c_int64]
    lib.ldg_efmsec_read.restype = C.c_int64
    lib.ldg_field_line_services.argtypes = [vp, C.c_int, vp, vp]
    lib.ldg_frames_line_services.argtypes = [vp, C.c_int, vp, C.c_int, vp]
    lib.ldg_flac_open.argtypes = [vp, C.c_char_p, C.POINTER(FlacInfo)]
    lib.ldg_flac_index.argtypes = [vp, C.c_int64, C.POINTER(FlacCounters)]
    lib.ldg_flac_frames.argtypes = [vp, vp, C.c_int64, vp, C.c_int64]
    lib.ldg_flac_read.argtypes = [vp, C.c_int64, C.c_int64, vp, C.c_int]
    lib.ldg_flac_capture.argtypes = [vp, C.c_int64, C.c_int64]
    lib.ldg_flac_close.argtypes = [vp]
    lib.ldg_version.restype = C.c_char_p
    lib.ldg_device_count.restype = C.c_int
    _lib = lib
    return lib


def device_memory(device=0):
    """(free, total) bytes of device memory (ldg_device_memory)."""
    f, t = C.c_int64(), C.c_int64()
    rc = load().ldg_device_memory(int(device), C.byref(f), C.byref(t))
    if rc != LDG_OK:
        raise LDGError('ldg_device_memory failed (%d)' % rc)
    return f.value, t.value


def _ptr(a, t=C.c_double):
    return a.ctypes.data_as(C.POINTER(t))


class LDGError(RuntimeError):
    pass


class PinnedBuffer:
    """Page-locked host memory (ldg_host_alloc) viewed as a numpy uint16 array; grows on
    demand.  A grown buffer keeps its old allocation alive (retired) until
    release_retired(): a view handed to a sink before the growth stays valid until the
    owner says the views are dead (GPUDecoder.decode: at its end)."""

    def __init__(self):
        self.lib = load()
        self.ptr, self.nbytes, self.arr = None, 0, None
        self.retired = []

    def view(self, count):
        nbytes = max(2 * count, 2)
        if nbytes > self.nbytes:
            if self.ptr is not None:
                self.retired.append(self.ptr)
            self.ptr, self.nbytes, self.arr = None, 0, None
            p = C.c_void_p()
            if self.lib.ldg_host_alloc(nbytes, C.byref(p)) != LDG_OK:
                raise LDGError('ldg_host_alloc(%d) failed' % nbytes)
            self.ptr, self.nbytes = p, nbytes
            self.arr = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint16)), shape=(nbytes // 2,))
        return self.arr[:count]

    def release_retired(self):
        for p in self.retired:
            self.lib.ldg_host_free(p)
        self.retired = []

    def free(self):
        self.release_retired()
        if self.ptr is not None:
            self.lib.ldg_host_free(self.ptr)
            self.ptr, self.nbytes, self.arr = None, 0, None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Context:
    """One libldgpu context (one GPU).  Owns device memory for ``max_reads`` field reads."""

    def __init__(self, system='NTSC', device=0, max_reads=32, max_frames=None):
        self.lib = load()
        if self.lib.ldg_device_count() <= 0:
            raise LDGError('no HIP device visible: the ldgpu decode path needs an MI355X (no CPU fallback)')
        cfg = Config(1 if system == 'PAL' else 0, device, max_reads, max_frames or max_reads)
        h = C.c_void_p()
        rc = self.lib.ldg_create(C.byref(cfg), C.byref(h))
        if rc != LDG_OK:
            raise LDGError('ldg_create failed (%d)' % rc)
        self.h = h
        self.system = system
        self.max_reads = max_reads
        self.max_frames = max_frames or max_reads
        self._keep = []
        self._pending = []          # read counts of the outstanding ldg_decode_reads_async calls

    def _check(self, rc, what):
        if rc != LDG_OK:
            raise LDGError('%s failed (%d): %s' % (what, rc, self.lib.ldg_last_error(self.h).decode()))

    def close(self):
        if self.h:
            self.lib.ldg_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_filters(self, params, tables):
        """params: dict of ldg_params fields; tables: dict name -> complex128/float64 array."""
        p = Params()
        for k, _ in Params._fields_:
            if k == 'codelines':
                for i, v in enumerate(params['codelines']):
                    p.codelines[i] = int(v)
            elif k != 'pad_':
                setattr(p, k, params[k])
        keep = {}
        f = Filters()
        for k, _ in Filters._fields_:
            a = tables.get(k)
            if a is None:
                setattr(f, k, C.POINTER(C.c_double)())
                continue
            if np.iscomplexobj(a):
                a = np.ascontiguousarray(a, dtype=np.complex128).view(np.float64)
            else:
                a = np.ascontiguousarray(a, dtype=np.float64)
            keep[k] = a
            setattr(f, k, _ptr(a))
        self._check(self.lib.ldg_set_filters(self.h, C.byref(p), C.byref(f)), 'ldg_set_filters')
        self.params = params

    def set_capture(self, raw, nsamples, fmt, first_sample=0, device_ptr=None):
        if device_ptr is not None:
            rc = self.lib.ldg_set_capture(self.h, C.c_void_p(device_ptr), nsamples, fmt, first_sample, 1)
        else:
            buf = np.frombuffer(raw, dtype=np.uint8) if not isinstance(raw, np.ndarray) else raw.view(np.uint8)
            buf = np.ascontiguousarray(buf)
            rc = self.lib.ldg_set_capture(self.h, buf.ctypes.data_as(C.c_void_p), nsamples, fmt, first_sample, 0)
        self._check(rc, 'ldg_set_capture')

    # ---- streamed capture (ldg_stream_*) -------------------------------------------
    def stream_open(self, path, fmt, ring_bytes, first_sample=0):
        """Stream the capture file at `path` through an HBM ring of ring_bytes (see
        include/ldgpu.h); replaces any resident capture."""
        self._check(self.lib.ldg_stream_open(self.h, os.fsencode(path), int(fmt), int(ring_bytes), int(first_sample)),
                    'ldg_stream_open')

    def stream_release(self, below_sample):
        self._check(self.lib.ldg_stream_release(self.h, int(below_sample)), 'ldg_stream_release')

    def stream_seek(self, first_sample):
        self._check(self.lib.ldg_stream_seek(self.h, int(first_sample)), 'ldg_stream_seek')

    def stream_window(self):
        """(lowest readable sample, highest block end a launch may reach, samples read so far,
        total samples)"""
        out = np.zeros(4, dtype=np.int64)
        self._check(self.lib.ldg_stream_window(self.h, out.ctypes.data), 'ldg_stream_window')
        return tuple(int(x) for x in out)

    def stream_stats(self):
        out = np.zeros(len(STREAM_STATS), dtype=np.float64)
        n = self.lib.ldg_stream_stats(self.h, out.ctypes.data, out.size)
        if n < 0:
            self._check(n, 'ldg_stream_stats')
        return dict(zip(STREAM_STATS[:n], (float(x) for x in out[:n])))

    def stream_close(self):
        self._check(self.lib.ldg_stream_close(self.h), 'ldg_stream_close')

    def decode_reads(self, starts, mtfs, slots=None):
        n = len(starts)
        s = np.ascontiguousarray(starts, dtype=np.int64)
        m = np.ascontiguousarray(mtfs, dtype=np.float64)
        sl = np.ascontiguousarray(slots if slots is not None else np.arange(n), dtype=np.int32)
        info = (FieldInfo * n)()
        self._check(self.lib.ldg_decode_reads(self.h, n, _ptr(s, C.c_int64), _ptr(m), _ptr(sl, C.c_int32), info),
                    'ldg_decode_reads')
        out = list(info)
        for _ in range(3):
            # a read whose odd-half park another demod workgroup overwrote (FS_MIGRATED) is void: decode it again
            redo = [i for i, x in enumerate(out) if x.status == FS_MIGRATED]
            if not redo:
                break
            again = self.decode_reads(s[redo], m[redo], sl[redo])
            for i, x in zip(redo, again):
                out[i] = x
        return out

    def decode_reads_async(self, starts, mtfs, slots, full=None):
        """Launch a decode (ldg_decode_reads_async2, up to 8 outstanding); decode_reads_wait()
        returns the records of the oldest outstanding one.  full: per read flags, READ_FULL
        (or True) exempts it from the video cut (set_video_cut; reads that came back FS_VCUT),
        READ_PROBE moves a predicted start to the sync peak a probe finds (the record's
        readsample is the start decoded).  Returns the flags as the library left them
        (READ_PROBE set exactly for the reads probed), or None."""
        s, m, sl = (np.ascontiguousarray(starts, dtype=np.int64), np.ascontiguousarray(mtfs, dtype=np.float64),
                    np.ascontiguousarray(slots, dtype=np.int32))
        f = None if full is None else np.ascontiguousarray(full, dtype=np.uint8)
        self._check(self.lib.ldg_decode_reads_async2(self.h, s.size, s.ctypes.data, m.ctypes.data, sl.ctypes.data,
                                                     None if f is None else f.ctypes.data),
                    'ldg_decode_reads_async2')
        self._pending.append(s.size)
        return f

    def set_video_cut(self, out_samples):
        """The demod skips the video / burst / pilot channels of blocks whose outputs start at
        or past out_samples (0: no cut); a field that needs them comes back FS_VCUT."""
        self._check(self.lib.ldg_set_video_cut(self.h, int(out_samples)), 'ldg_set_video_cut')

    def decode_reads_wait(self):
        n = self._pending[0]
        info = (FieldInfo * n)()
        self._check(self.lib.ldg_decode_reads_wait(self.h, info), 'ldg_decode_reads_wait')
        self._pending.pop(0)
        return list(info)

    def field_audio(self, slots, offsets):
        n = len(slots)
        stride = 2048
        pcm = np.zeros((max(n, 1), stride), dtype=np.int16)
        counts = np.zeros(max(n, 1), dtype=np.int32)
        nxt = np.zeros(max(n, 1), dtype=np.float64)
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        of = np.ascontiguousarray(offsets, dtype=np.float64)
        self._check(self.lib.ldg_field_audio(self.h, n, _ptr(sl, C.c_int32), _ptr(of), _ptr(pcm, C.c_int16), stride,
                                             _ptr(counts, C.c_int32), _ptr(nxt)), 'ldg_field_audio')
        return pcm[:n], counts[:n], nxt[:n]

    def field_audio_async(self, slots, offsets):
        """Launch ldg_field_audio_async; field_audio_collect() returns what field_audio would."""
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        of = np.ascontiguousarray(offsets, dtype=np.float64)
        self._check(self.lib.ldg_field_audio_async(self.h, sl.size, sl.ctypes.data, of.ctypes.data),
                    'ldg_field_audio_async')
        self._audio_n = sl.size

    def field_audio_collect(self):
        n = self._audio_n
        stride = 2048
        pcm = np.zeros((max(n, 1), stride), dtype=np.int16)
        counts = np.zeros(max(n, 1), dtype=np.int32)
        nxt = np.zeros(max(n, 1), dtype=np.float64)
        self._check(self.lib.ldg_field_audio_collect(self.h, pcm.ctypes.data, stride, counts.ctypes.data,
                                                     nxt.ctypes.data), 'ldg_field_audio_collect')
        return pcm[:n], counts[:n], nxt[:n]

    def archive_fields(self, slots, first):
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        self._check(self.lib.ldg_archive_fields(self.h, sl.size, sl.ctypes.data, int(first)), 'ldg_archive_fields')

    def archive_audio(self, entries, offsets, packed=False):
        """ldg_field_audio over archive entries -> (pcm[n, 2048], counts, next offsets); packed:
        pcm is one flat array, the fields' 2 * counts samples one after another."""
        n = len(entries)
        stride = 0 if packed else 2048
        pcm = np.empty(max(n, 1) * 2048, dtype=np.int16) if packed else np.zeros((max(n, 1), stride), dtype=np.int16)
        counts = np.zeros(max(n, 1), dtype=np.int32)
        nxt = np.zeros(max(n, 1), dtype=np.float64)
        e = np.ascontiguousarray(entries, dtype=np.int64)
        o = np.ascontiguousarray(offsets, dtype=np.float64)
        self._check(self.lib.ldg_archive_audio(self.h, n, e.ctypes.data, o.ctypes.data, pcm.ctypes.data, stride,
                                               counts.ctypes.data, nxt.ctypes.data), 'ldg_archive_audio')
        if packed:
            return pcm[:int(2 * np.maximum(counts[:n], 0).sum())], counts[:n], nxt[:n]
        return pcm[:n], counts[:n], nxt[:n]

    def assemble_frames_device(self, tops, bottoms):
        """Assemble frames into the context's device frame buffer (no host copy)."""
        n = len(tops)
        t = np.ascontiguousarray(tops, dtype=np.int32)
        b = np.ascontiguousarray(bottoms, dtype=np.int32)
        self._check(self.lib.ldg_assemble_frames(self.h, n, _ptr(t, C.c_int32), _ptr(b, C.c_int32),
                                                 C.POINTER(C.c_uint16)(), 1), 'ldg_assemble_frames')

    def assemble_frames(self, tops, bottoms, W, H):
        n = len(tops)
        out = np.zeros((max(n, 1), H * W), dtype=np.uint16)
        t = np.ascontiguousarray(tops, dtype=np.int32)
        b = np.ascontiguousarray(bottoms, dtype=np.int32)
        self._check(self.lib.ldg_assemble_frames(self.h, n, _ptr(t, C.c_int32), _ptr(b, C.c_int32),
                                                 _ptr(out, C.c_uint16), 0), 'ldg_assemble_frames')
        return out[:n]

    def debug(self, slot, what, dtype, count):
        a = np.zeros(count, dtype=dtype)
        rc = self.lib.ldg_debug_read(self.h, slot, what, a.ctypes.data_as(C.c_void_p), a.nbytes)
        if rc < 0:
            raise LDGError('ldg_debug_read(%d,%d) -> %d' % (slot, what, rc))
        return a[:rc // a.itemsize]

    def rf_table(self, mtf):
        """The demod's RF filter RFVideo * MTF**mtf (complex128[16384], natural bin order)."""
        a = np.zeros(2 * 16384, dtype=np.float64)
        rc = self.lib.ldg_debug_rf_table(self.h, float(mtf), a.ctypes.data_as(C.c_void_p))
        if rc != LDG_OK:
            raise LDGError('ldg_debug_rf_table(%r) -> %d' % (mtf, rc))
        return a.view(np.complex128)

    def comb_ntsc(self, frames):
        """2D NTSC comb (comb-ntsc.cxx dim=2): n x (525, 910) uint16 frames -> n x (480, 744, 3) rgb48
        (comb_lines x comb_width with -v / -W).  State (burst-level EMA, -W's Y-NR history)
        carries across calls like one reference comb process."""
        f = np.ascontiguousarray(frames, dtype=np.uint16).reshape(-1, 525 * 910)
        out = np.zeros((f.shape[0], self.comb_lines, self.comb_width, 3), dtype=np.uint16)
        self._check(self.lib.ldg_comb_ntsc(self.h, f.shape[0], f.ctypes.data_as(C.c_void_p),
                                           out.ctypes.data_as(C.c_void_p), 0), 'ldg_comb_ntsc')
        return out

    def comb_ntsc3d(self, frames, core_ire=-1.0, range_ire=-1.0):
        """3D NTSC comb, comb-ntsc -d 3 -F (or, after comb_set_opts(opticalflow=True), -d 3 with
        the build-defined optical flow): n x (525, 910) uint16 frames in, the rgb48 frames that
        now have both neighbours out (none for a process's first two frames)."""
        f = np.ascontiguousarray(frames, dtype=np.uint16).reshape(-1, 525 * 910)
        out = np.zeros((f.shape[0], self.comb_lines, self.comb_width, 3), dtype=np.uint16)
        n_out = C.c_int(0)
        self._check(self.lib.ldg_comb_ntsc3d(self.h, f.shape[0], f.ctypes.data_as(C.c_void_p),
                                             out.ctypes.data_as(C.c_void_p), C.byref(n_out), core_ire, range_ire),
                    'ldg_comb_ntsc3d')
        return out[:n_out.value]

    def comb_pal(self, frames):
        """PAL Y/C decoder (build-defined, see include/ldgpu.h): n x (625, 1135) uint16 frames ->
        n x (576, 1057, 3) rgb48."""
        f = np.ascontiguousarray(frames, dtype=np.uint16).reshape(-1, 625 * 1135)
        out = np.zeros((f.shape[0], 576, 1057, 3), dtype=np.uint16)
        self._check(self.lib.ldg_comb_pal(self.h, f.shape[0], f.ctypes.data_as(C.c_void_p),
                                          out.ctypes.data_as(C.c_void_p)), 'ldg_comb_pal')
        return out

    def comb_pal_stages(self):
        """The PAL Y/C decoder's buffers as its last launch left them (ldg_debug_read 80..84), for
        that launch's m frames (the last chunk of at most max_frames of a longer call): cv
        [m, 601, 1136] SplitIQ's signed chroma of lines 24..624, angle [m, 625] the burst angles
        (degrees), phase [m] the V-switch votes, abl [m, 579] the burst-level EMA line 44 + j
        used, state the EMA carried into the next call.  LDGError before any PAL call."""
        phase = self.debug(0, 82, np.int32, self.max_frames)
        m = phase.size
        return dict(cv=self.debug(0, 80, np.float64, m * 601 * 1136).reshape(m, 601, 1136),
                    angle=self.debug(0, 81, np.float64, m * 625).reshape(m, 625), phase=phase,
                    abl=self.debug(0, 83, np.float64, m * 579).reshape(m, 579),
                    state=float(self.debug(0, 84, np.float64, 1)[0]))

    def comb_ntsc_device(self, n):
        """Comb the first n frames of the context's device frame buffer (ldg_assemble_frames
        with out=NULL) into the context's device rgb buffer (benchmark mode)."""
        self._check(self.lib.ldg_comb_ntsc(self.h, n, None, None, 1), 'ldg_comb_ntsc')

    def comb_ntsc_async(self, n):
        """ldg_comb_ntsc_async: comb the context's first n device frames on the comb stream."""
        self._check(self.lib.ldg_comb_ntsc_async(self.h, n), 'ldg_comb_ntsc_async')

    def comb_async(self, n):
        """ldg_comb_async: the context's system's comb (NTSC 2D, or the PAL Y/C decoder) over
        its first n device frames, on the comb stream."""
        self._check(self.lib.ldg_comb_async(self.h, n), 'ldg_comb_async')

    def demod_isolated(self, slots, iters, variant=0):
        """Mean HIP-event ms of one demod-only launch over these live slots: variant 0
        ldg_k_demod_iso (every block in full), 1 ldg_k_demod_iso_cut (the shipped body)."""
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        ms = C.c_double()
        self._check(self.lib.ldg_demod_isolated_ex(self.h, sl.size, sl.ctypes.data, iters, variant, C.byref(ms)),
                    'ldg_demod_isolated_ex')
        return ms.value

    def output_async(self, tops, bottoms, tbc, rgb=None):
        """ldg_output_async: frames (and the 2D comb's rgb48 when rgb is given) into the host
        arrays `tbc` / `rgb` (pinned: PinnedBuffer views) on the output stream; returns at once,
        output_wait() waits for the copies."""
        n = len(tops)
        t = np.ascontiguousarray(tops, dtype=np.int32)
        b = np.ascontiguousarray(bottoms, dtype=np.int32)
        self._out_keep = (t, b)
        self._check(self.lib.ldg_output_async(self.h, n, t.ctypes.data, b.ctypes.data, tbc.ctypes.data,
                                              rgb.ctypes.data if rgb is not None else None), 'ldg_output_async')

    def output_wait(self):
        self._check(self.lib.ldg_output_wait(self.h), 'ldg_output_wait')

    def sync(self):
        self._check(self.lib.ldg_sync(self.h), 'ldg_sync')

    def comb_set_state(self, aburstlev):
        self._check(self.lib.ldg_comb_set_state(self.h, float(aburstlev)), 'ldg_comb_set_state')

    comb_lines = 480                 # rows per rgb48 frame (comb-ntsc -v: 525)
    comb_width = 744                 # pixels per rgb48 row (comb-ntsc -W: 910)

    def comb_set_opts(self, **opts):
        """comb-ntsc's options (ldg_comb_set_opts; keys of COMB_DEFAULTS, values as on the
        reference's command line); no arguments restores the defaults."""
        o = dict(COMB_DEFAULTS)
        for k, v in opts.items():
            if k not in o:
                raise TypeError('unknown comb option %s' % k)
            o[k] = v
        c = CombOpts(**{k: (int(v) if isinstance(v, bool) else v) for k, v in o.items()})
        self._check(self.lib.ldg_comb_set_opts(self.h, C.byref(c)), 'ldg_comb_set_opts')
        self.comb_lines = int(o['linesout'])
        self.comb_width = 910 if o['wide'] else 744

    # ---- RF dropouts (build-defined; include/ldgpu.h) ---------------------------------
    def set_dropout_opts(self, opts=None, **kw):
        """ldg_set_dropout_opts: None switches the feature off; a dict (or keywords) of
        ldg_dropout_opts fields over the system's defaults switches it on.  Returns the
        options in force (None: off)."""
        if opts is None and not kw:
            self._check(self.lib.ldg_set_dropout_opts(self.h, None), 'ldg_set_dropout_opts')
            return None
        o = dropout_defaults(self.system)
        for k, v in dict(opts or {}, **kw).items():
            if k not in o:
                raise TypeError('unknown dropout option %s' % k)
            o[k] = v
        c = DropoutOpts(float(o['lo_ire']), float(o['hi_ire']), int(o['merge_gap']), int(o['min_flagged']),
                        int(o['pad']), int(bool(o['conceal'])))
        self._check(self.lib.ldg_set_dropout_opts(self.h, C.byref(c)), 'ldg_set_dropout_opts')
        return o

    def field_dropouts(self, slots):
        """ldg_field_dropouts: per slot an int16 array [count, 3] of (row, startx, endx) in
        (row, startx) order, or None for a field that is not valid."""
        if len(slots) > self.max_reads:               # (a call takes at most max_reads slots)
            return [r for i in range(0, len(slots), self.max_reads)
                    for r in self.field_dropouts(slots[i:i + self.max_reads])]
        n = len(slots)
        stride = MAX_DROPOUTS_PER_LINE * MAX_LINES
        out = np.empty((max(n, 1), stride, 4), dtype=np.int16)
        counts = np.zeros(max(n, 1), dtype=np.int32)
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        self._check(self.lib.ldg_field_dropouts(self.h, n, sl.ctypes.data, out.ctypes.data, stride, counts.ctypes.data),
                    'ldg_field_dropouts')
        return [None if counts[i] < 0 else out[i, :counts[i], :3].copy() for i in range(n)]

    # ---- NTSC line services (build-defined; include/ldgpu.h) -----
    def field_line_services(self, slots):
        """ldg_field_line_services: per live slot the record (line_records) of its field (white_count
        -1: the field is not valid)."""
        if len(slots) > self.max_reads:               # (a call takes at most max_reads slots)
            return [r for i in range(0, len(slots), self.max_reads)
                    for r in self.field_line_services(slots[i:i + self.max_reads])]
        n = len(slots)
        out = np.zeros(max(n, 1), dtype=np.dtype(LineServices))
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        self._check(self.lib.ldg_field_line_services(self.h, n, sl.ctypes.data, out.ctypes.data),
                    'ldg_field_line_services')
        return line_records(out[:n])

    def frames_line_services(self, frames=None, device_ptr=None, n=None):
        """ldg_frames_line_services over packed 910 x 525 frames: a host array of n frames, or n
        frames at a device pointer.  Returns [n][2] records (top field, bottom field)."""
        if device_ptr is None:
            fr = np.ascontiguousarray(frames, dtype=np.uint16).reshape(-1, 525 * 910)
            n, ptr = fr.shape[0], fr.ctypes.data
        else:
            ptr = int(device_ptr)
        out = np.zeros((max(n, 1), 2), dtype=np.dtype(LineServices))
        self._check(self.lib.ldg_frames_line_services(self.h, n, ptr, int(device_ptr is not None), out.ctypes.data),
                    'ldg_frames_line_services')
        recs = line_records(out[:n])
        return [recs[2 * i:2 * i + 2] for i in range(n)]

    def comb_reset(self):
        self._check(self.lib.ldg_comb_reset(self.h), 'ldg_comb_reset')

    # ---- disc stacking (build-defined; include/ldgpu.h) ----------
    def stack_frames(self, sources, present=None, runs=None, counts=None, mode='smart-mean', threshold=3840):
        """ldg_stack_frames over any number of frames, max_frames a call.  sources: per source
        an array of n frames (any shape of n * rows * pixels uint16), or None for a source that
        is present nowhere; present: bool [n, n_src] (None: every source everywhere); runs int16
        [n, n_src, 2, MAX_LINES, 8, 2] and counts int32 [n, n_src, 2, MAX_LINES] (both None: no
        runs).  mode: a key of STACK_MODES or its value.  Returns uint16 [n, rows, pixels]."""
        H, W = FRAME_SHAPE[self.system]
        n_src = len(sources)
        srcs = [None if a is None else np.ascontiguousarray(a, dtype=np.uint16).reshape(-1, H * W) for a in sources]
        ns = {a.shape[0] for a in srcs if a is not None}
        if len(ns) > 1:
            raise ValueError('stack_frames: the sources hold different numbers of frames (%s)' % sorted(ns))
        if present is None:
            if not ns:
                raise ValueError('stack_frames: no source given')
            present = np.ones((ns.pop(), n_src), dtype=np.uint8)
        pres = np.ascontiguousarray(np.asarray(present) != 0, dtype=np.uint8).reshape(-1, max(n_src, 1))
        n = pres.shape[0]
        if (runs is None) != (counts is None):
            raise ValueError('stack_frames: runs and counts go together')
        if runs is not None:
            runs = np.ascontiguousarray(runs, dtype=np.int16).reshape(n, n_src, 2, MAX_LINES, MAX_DROPOUTS_PER_LINE, 2)
            counts = np.ascontiguousarray(counts, dtype=np.int32).reshape(n, n_src, 2, MAX_LINES)
        out = np.empty((n, H, W), dtype=np.uint16)
        step = self.max_frames
        for f0 in range(0, n, step):
            m = min(step, n - f0)
            ptrs = (C.c_void_p * max(n_src, 1))(*[None if a is None else a[f0:].ctypes.data for a in srcs])
            self._check(self.lib.ldg_stack_frames(
                self.h, m, n_src, ptrs, pres[f0:].ctypes.data,
                None if runs is None else runs[f0:].ctypes.data, None if counts is None else counts[f0:].ctypes.data,
                int(STACK_MODES.get(mode, mode)), int(threshold), out[f0:].ctypes.data), 'ldg_stack_frames')
        return out

    def conceal_frames(self, frames, runs, counts, nrows):
        """ldg_conceal_frames: the concealed copy of n frames.  runs int16 [n, 2, MAX_LINES, 8, 2],
        counts int32 [n, 2, MAX_LINES], nrows int32 [n, 2] (the two fields' line counts)."""
        H, W = FRAME_SHAPE[self.system]
        out = np.array(frames, dtype=np.uint16, order='C').reshape(-1, H, W)
        n = out.shape[0]
        runs = np.ascontiguousarray(runs, dtype=np.int16).reshape(n, 2, MAX_LINES, MAX_DROPOUTS_PER_LINE, 2)
        counts = np.ascontiguousarray(counts, dtype=np.int32).reshape(n, 2, MAX_LINES)
        nrows = np.ascontiguousarray(nrows, dtype=np.int32).reshape(n, 2)
        self._check(self.lib.ldg_conceal_frames(self.h, n, out.ctypes.data, runs.ctypes.data, counts.ctypes.data,
                                                nrows.ctypes.data), 'ldg_conceal_frames')
        return out

    def stack_stats(self):
        """ldg_stack_stats: seconds in ldg_stack_frames' copies in, kernel and copies out; calls."""
        out = np.zeros(len(STACK_STATS), dtype=np.float64)
        n = self.lib.ldg_stack_stats(self.h, out.ctypes.data, out.size)
        if n < 0:
            self._check(n, 'ldg_stack_stats')
        return dict(zip(STACK_STATS[:n], (float(x) for x in out[:n])))

    # ---- EFM run lengths (build-defined; include/ldgpu.h) --------
    def efm_set_opts(self, taps, **opts):
        """ldg_efm_set_opts: the 255 low-pass taps and ldg_efm_opts fields over the defaults.
        Returns the options in force."""
        o = efm_defaults()
        for k, v in opts.items():
            if k not in o:
                raise TypeError('unknown EFM option %s' % k)
            o[k] = v
        c = EfmOpts(float(o['fs']), float(o['alpha']), float(o['beta']), float(o['delta']), int(bool(o['keep_debug'])), 0)
        t = np.ascontiguousarray(taps, dtype=np.float64)
        self._check(self.lib.ldg_efm_set_opts(self.h, C.byref(c), t.ctypes.data, t.size), 'ldg_efm_set_opts')
        return o

    def efm_extract(self, raw, fmt, first_sample, file_nsamples, seg_lo, seg_hi, device_ptr=None, nbytes=None):
        """ldg_efm_extract: (bytes uint8[n], per-segment list of dicts).  raw: the window's bytes
        (buffer or uint8 array) from first_sample; or device_ptr / nbytes for a window in HBM."""
        nseg = max(int(seg_hi) - int(seg_lo), 0)
        cap = nseg * (EFM_SEG // 4) + (1 << 14)
        out = np.empty(cap, dtype=np.uint8)
        segs = (EfmSeg * max(nseg, 1))()
        n = C.c_int64(0)
        if device_ptr is not None:
            ptr, nb = C.c_void_p(device_ptr), int(nbytes)
        else:
            buf = np.frombuffer(raw, dtype=np.uint8) if not isinstance(raw, np.ndarray) else raw.view(np.uint8)
            buf = np.ascontiguousarray(buf)
            ptr, nb = buf.ctypes.data_as(C.c_void_p), buf.size
        self._check(self.lib.ldg_efm_extract(self.h, ptr, nb, int(fmt), int(first_sample), int(file_nsamples),
                                             int(seg_lo), int(seg_hi), out.ctypes.data, cap, C.byref(n), segs),
                    'ldg_efm_extract')
        return out[:n.value].copy(), [{k: getattr(segs[i], k) for k, _ in EfmSeg._fields_} for i in range(nseg)]

    def efm_debug(self, what):
        """ldg_efm_debug_read of the last efm_extract: 'z' -> (first m, float64 z), 'times' ->
        float64 crossing times."""
        w = {'z': 0, 'times': 1}[what]
        first = C.c_int64(0)
        a = np.zeros(1 << 16, dtype=np.float64)
        while True:
            rc = self.lib.ldg_efm_debug_read(self.h, w, a.ctypes.data, a.nbytes, C.byref(first))
            if rc < 0:
                raise LDGError('ldg_efm_debug_read(%s) -> %d' % (what, rc))
            if rc < a.nbytes:
                break
            a = np.zeros(a.size * 4, dtype=np.float64)
        a = a[:rc // 8].copy()
        return (int(first.value), a) if what == 'z' else a

    # ---- EFM decode (build-defined; include/ldgpu.h) -------------
    def efmdec_set_table(self, inverse):
        """ldg_efmdec_set_table: the 16384-entry inverse code table (uint16); resets the stream."""
        t = np.ascontiguousarray(inverse, dtype=np.uint16)
        self._check(self.lib.ldg_efmdec_set_table(self.h, t.ctypes.data, t.size), 'ldg_efmdec_set_table')

    def efmdec_reset(self):
        self._check(self.lib.ldg_efmdec_reset(self.h), 'ldg_efmdec_reset')

    def efmdec_feed(self, rl, final=False):
        """ldg_efmdec_feed: the next run lengths (uint8 array) -> ldg_efmdec_info as a dict."""
        buf = np.ascontiguousarray(rl, dtype=np.uint8)
        info = EfmdecInfo()
        self._check(self.lib.ldg_efmdec_feed(self.h, buf.ctypes.data, buf.size, int(bool(final)), C.byref(info)),
                    'ldg_efmdec_feed')
        return {k: getattr(info, k) for k, _ in EfmdecInfo._fields_}

    def efmdec_read(self, what, count):
        """ldg_efmdec_read of the last efmdec_feed: EFMDEC_ARRAYS[what] for `count` samples
        (pcm, flags) or frames (the others) -> (index of the first, array)."""
        w, dt, per = EFMDEC_ARRAYS[what]
        a = np.zeros((int(count), per) if per > 1 else int(count), dtype=dt)
        first = C.c_int64(0)
        if a.size == 0:
            return 0, a
        rc = self.lib.ldg_efmdec_read(self.h, w, a.ctypes.data, a.nbytes, C.byref(first))
        if rc != a.nbytes:
            raise LDGError('ldg_efmdec_read(%s) -> %d, expected %d bytes' % (what, rc, a.nbytes))
        return int(first.value), a

    # ---- EFM data sectors (build-defined; include/ldgpu.h) -------
    def efmsec_enable(self, on=True):
        """ldg_efmsec_enable: efmdec_feed hands its frames to the sector stage (or no longer)."""
        self._check(self.lib.ldg_efmsec_enable(self.h, int(bool(on))), 'ldg_efmsec_enable')

    def efmsec_reset(self):
        self._check(self.lib.ldg_efmsec_reset(self.h), 'ldg_efmsec_reset')

    def efmsec_feed(self, data, erased, final=False):
        """ldg_efmsec_feed: the next bytes and their erasure flags (uint8 arrays of one size) ->
        ldg_efmsec_info as a dict."""
        by = np.ascontiguousarray(data, dtype=np.uint8)
        er = np.ascontiguousarray(erased, dtype=np.uint8)
        if by.shape != er.shape or by.ndim != 1:
            raise ValueError('efmsec_feed: bytes and flags are flat arrays of one size')
        info = EfmsecInfo()
        self._check(self.lib.ldg_efmsec_feed(self.h, by.ctypes.data, er.ctypes.data, by.size, int(bool(final)),
                                             C.byref(info)), 'ldg_efmsec_feed')
        return {k: getattr(info, k) for k, _ in EfmsecInfo._fields_}

    def efmsec_last_info(self):
        info = EfmsecInfo()
        self._check(self.lib.ldg_efmsec_last_info(self.h, C.byref(info)), 'ldg_efmsec_last_info')
        return {k: getattr(info, k) for k, _ in EfmsecInfo._fields_}

    def efmsec_read(self, what, count):
        """ldg_efmsec_read of the stage's last call: EFMSEC_ARRAYS[what] for `count` sectors
        (bytes, erased: bytes)."""
        w, dt, per = EFMSEC_ARRAYS[what]
        a = np.zeros((int(count), per) if per > 1 else int(count), dtype=dt)
        if a.size == 0:
            return a
        rc = self.lib.ldg_efmsec_read(self.h, w, a.ctypes.data, a.nbytes)
        if rc != a.nbytes:
            raise LDGError('ldg_efmsec_read(%s) -> %d, expected %d bytes' % (what, rc, a.nbytes))
        return a

    # ---- profiling / tooling -------------------------------------------------------
    def profile(self, on=True):
        """on: True (every kernel), 'demod' (the demod only), False."""
        mode = 2 if on == 'demod' else (1 if on else 0)
        self._check(self.lib.ldg_profile_enable(self.h, mode), 'ldg_profile_enable')

    def profile_spans(self):
        """(count, total ms) of the demod launches' execution spans since profile(on)."""
        t, n = C.c_double(0), C.c_int64(0)
        self._check(self.lib.ldg_profile_spans(self.h, C.byref(t), C.byref(n)), 'ldg_profile_spans')
        return int(n.value), float(t.value)

    def profile_spans_union(self):
        """(count, ms) of demod launches and the time at least one of them was executing."""
        t, n = C.c_double(0), C.c_int64(0)
        self._check(self.lib.ldg_profile_spans_union(self.h, C.byref(t), C.byref(n)), 'ldg_profile_spans_union')
        return int(n.value), float(t.value)

    def profile_span_table(self):
        """float64[n, 4]: every profiled demod launch in issue order -- execution start, end
        and host issue time, ms on the device clock from the first start, and the issue time
        in ms of the host's monotonic clock (time.perf_counter() * 1e3; ldg_profile_span_table)."""
        out = np.zeros((8192, 4), dtype=np.float64)
        n = self.lib.ldg_profile_span_table(self.h, out.ctypes.data, out.shape[0])
        if n < 0:
            self._check(n, 'ldg_profile_span_table')
        return out[:n]

    def profile_stats(self):
        arr = (KernelStat * 64)()
        n = self.lib.ldg_profile_read(self.h, arr, 64)
        return {arr[i].name.decode(): (int(arr[i].launches), float(arr[i].total_ms)) for i in range(min(n, 64))}

    def synth(self, nsamples, fmt=0, first_frame=1, clv=False, seed=20181015, noise=0.02, start_line=100,
              start_sample=0):
        """Generate a synthetic NTSC capture straight into this context's HBM capture buffer.
        start_sample: generate samples [start_sample, start_sample + nsamples) of the capture
        (a shard's window; line timing and frame codes follow the whole capture's)."""
        import scipy.signal as sps
        from .synth import NTSC, FrameCodes, emphasis_filter, FS
        fir = np.ascontiguousarray(sps.firwin(63, 4.4e6 / (FS / 2)), dtype=np.float64)
        b, a = emphasis_filter(NTSC)
        emph = np.array([b[0], b[1], a[1]], dtype=np.float64)
        spl = FS * NTSC['line_us'] / 1e6
        start_line = start_line + start_sample / spl
        nframes = int((nsamples / spl + start_line) // 525) + 2
        fc = FrameCodes(first_frame, clv, 30)
        codes = np.array([fc.codes(k) for k in range(nframes)], dtype=np.uint32).reshape(-1)
        p = SynthParams(fmt, 0, nsamples, seed, noise, start_line)
        self._check(self.lib.ldg_synth_capture(self.h, C.byref(p), _ptr(fir), _ptr(emph), _ptr(codes, C.c_uint32),
                                               nframes), 'ldg_synth_capture')

    def capture_copy_to_device(self, dst_ptr, offset, nbytes):
        """Copy resident capture bytes into a device buffer (e.g. a torch CUDA tensor)."""
        n = self.lib.ldg_capture_download(self.h, C.c_void_p(dst_ptr), offset, nbytes)
        if n != nbytes:
            raise LDGError('ldg_capture_download -> %d' % n)

    def capture_download(self, offset, nbytes):
        a = np.zeros(nbytes, dtype=np.uint8)
        n = self.lib.ldg_capture_download(self.h, a.ctypes.data_as(C.c_void_p), offset, nbytes)
        if n < 0:
            raise LDGError('ldg_capture_download -> %d' % n)
        return a[:n]


def tail_plan(n_out, n_audio, n_audio2, vcut):
    """ldg_tail_plan: (acut1, acut2, live audio phase-2 blocks, demod blocks making audio
    slices, demod blocks storing demod_05) of a read under the video cut vcut (0: none);
    acut1 / acut2 are None where the audio is not trimmed.  Host code, no device needed."""
    out = np.zeros(5, dtype=np.int64)
    rc = load().ldg_tail_plan(int(n_out), int(n_audio), int(n_audio2), int(vcut), out.ctypes.data)
    if rc != 0:
        raise ValueError('ldg_tail_plan: %d' % rc)
    a1, a2, l2, l1, l05 = (int(v) for v in out)
    return (None if a1 < 0 else a1, None if a2 < 0 else a2, l2, l1, l05)


def div_const(x, c, guarded=True):
    """ldg_div_const: x / c by the row kernels' product-and-two-FMAs sequence (guarded: +-0,
    +-inf and NaN as the division gives them).  ValueError when c has no usable reciprocal.
    Host code, no device needed."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty_like(x)
    if load().ldg_div_const(x.ctypes.data, x.size, float(c), int(bool(guarded)), out.ctypes.data) != 0:
        raise ValueError('ldg_div_const: no reciprocal form for %r' % c)
    return out


def divconst_ok(c):
    """True when ldg_div_const (and the kernels) divide by c through its reciprocal."""
    return load().ldg_div_const(None, 0, float(c), 1, None) == 0


def audio_reach(lines, linecount, linelen):
    """ldg_audio_reach: (lowest, highest) input-sample position downscale_audio can form
    from a field's final line locations.  Host code, no device needed."""
    ll = np.ascontiguousarray(lines, dtype=np.float64)
    out = np.zeros(2, dtype=np.float64)
    rc = load().ldg_audio_reach(ll.ctypes.data, ll.size, int(linecount), float(linelen), out.ctypes.data)
    if rc != 0:
        raise ValueError('ldg_audio_reach: %d' % rc)
    return float(out[0]), float(out[1])


def audio_offsets(o0, linecounts, line_period):
    """ldg_audio_offsets: [o0, o1, ..., on] of downscale_audio's 48 kHz offset chain over
    the fields' line counts (host code in the library, no device needed)."""
    lc = np.ascontiguousarray(linecounts, dtype=np.float64)
    out = np.zeros(lc.size + 1, dtype=np.float64)
    rc = load().ldg_audio_offsets(float(o0), lc.size, lc.ctypes.data, float(line_period), out.ctypes.data)
    if rc != 0:
        raise IndexError('downscale_audio: empty tick range (the reference raises here)')
    return out.tolist()


class CXExpander:
    """cx-expander (cx-expander.cxx:34-92) through ldg_cx_process: host code, no device needed.
    State carries across process() calls like one cx process."""

    def __init__(self):
        self.lib = load()
        h = C.c_void_p()
        if self.lib.ldg_cx_create(C.byref(h)) != LDG_OK:
            raise LDGError('ldg_cx_create failed')
        self.h = h

    def process(self, stereo_u16):
        """(n, 2) or flat interleaved uint16 -> (n, 2) uint16."""
        a = np.ascontiguousarray(stereo_u16, dtype=np.uint16).reshape(-1, 2)
        out = np.empty_like(a)
        if self.lib.ldg_cx_process(self.h, a.shape[0], a.ctypes.data, out.ctypes.data) != LDG_OK:
            raise LDGError('ldg_cx_process failed')
        return out

    def __del__(self):
        if getattr(self, 'h', None):
            self.lib.ldg_cx_destroy(self.h)
            self.h = None
