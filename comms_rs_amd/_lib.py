"""ctypes loader of libcomms_hip.so -- the C ABI declared in include/comms_hip.h.

The library is built in-tree by comms_rs_amd/csrc/Makefile (hipcc, gfx950).
There is no CPU fallback: if the library is missing this module raises, and
every create call fails with COMMS_ERR_DEVICE when no MI355X is visible.
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
# COMMS_HIP_LIB selects another build of the same ABI (e.g. lib/libcomms_hip_diag.so, `make diag`)
LIB_PATH = os.environ.get("COMMS_HIP_LIB") or os.path.join(_HERE, "lib", "libcomms_hip.so")
CSRC = os.path.join(_HERE, "csrc")

COMMS_OK, COMMS_ERR_ARG, COMMS_ERR_DEVICE = 0, 1, 2
FIR_AUTO, FIR_DIRECT, FIR_OVERLAP_SAVE, FIR_OS1024, FIR_OS4096, FIR_OS16K, FIR_OS1024_FIXED = 0, 1, 2, 3, 4, 5, 6
IQ_C32, IQ_I16, IQ_U8 = 0, 1, 2
SYM_C32, SYM_BITS = 0, 1        # comms_pulse_set_input_format, comms_chain_set_output_format
SYM_LLR = 3                     # comms_deframe_set_output_format only
DEFRAME_NORMALISE = 1           # comms_deframe_create: flags
CONV_TERMINATED, CONV_TRUNCATED = 0, 1  # comms_convenc_create, comms_viterbi_create: flags
RATEMATCH_TX, RATEMATCH_RX = 0, 1  # comms_ratematch_get_kernel: direction
CRC_ATTACH, CRC_CHECK = 0, 1    # comms_crc_get_kernel: direction
DEMAP_TABLE = 1                 # comms_demap_create: flags
OFDM_NULL, OFDM_DATA, OFDM_PILOT = 0, 1, 2  # comms_ofdm_create: carrier_kind
OFDM_CPE = 1                    # comms_ofdm_create: flags
OFDM_MOD, OFDM_DEMOD = 0, 1     # comms_ofdm_get_kernel: direction
BITS_U8, BITS_PACKED = 0, 1     # comms_prns_run formats
RESAMPLE_F32, RESAMPLE_C32 = 4, 8  # comms_resample_create: bytes per sample
CHANNELIZER_CHANNEL_MAJOR, CHANNELIZER_FRAME_MAJOR = 0, 1  # comms_channelizer_create: layout
SPECTRUM_NATURAL, SPECTRUM_CENTRED = 0, 1  # comms_spectrum_create: order
SPECTRUM_CHUNK = 32             # segments per partial sum of a spectrum row
WINDOW_RECT, WINDOW_HANN, WINDOW_HAMMING, WINDOW_BLACKMAN = 0, 1, 2, 3  # comms_window_taps: kind
STREAM_HANDLE = C.c_void_p(-1).value  # COMMS_STREAM_HANDLE: the handle's own stream


def build(force=False):
    """Compile every HIP source for gfx950 into lib/libcomms_hip.so (needs hipcc, no GPU)."""
    os.makedirs(os.path.join(_HERE, "lib"), exist_ok=True)
    if force:
        subprocess.check_call(["make", "-C", CSRC, "-s", "clean"])
    subprocess.check_call(["make", "-C", CSRC, "-s", "-j8"])
    return LIB_PATH


class CommsError(RuntimeError):
    """Non-zero comms_status_t.  code 1 ~ NodeError::DataError, 2 ~ NodeError::PermanentError."""

    def __init__(self, code, msg):
        super().__init__("comms_hip status %d: %s" % (code, msg))
        self.code = code


_lib = None

_sz, _i32, _u32, _u64, _f64, _vp = C.c_size_t, C.c_int32, C.c_uint32, C.c_uint64, C.c_double, C.c_void_p
_pp = C.POINTER(C.c_void_p)
_psz = C.POINTER(C.c_size_t)

# name -> argtypes; every one returns comms_status_t unless listed in _OTHER
_PROTOS = {
    "comms_device_count": [C.POINTER(_i32)],
    "comms_device_info": [_i32, C.c_char_p, _sz, C.POINTER(_i32), C.POINTER(_u64)],
    "comms_buf_alloc": [_sz, _i32, _pp],
    "comms_buf_retain": [_vp],
    "comms_buf_release": [_vp],
    "comms_buf_upload": [_vp, _sz, _vp, _sz],
    "comms_buf_download": [_vp, _sz, _vp, _sz],
    "comms_buf_pool_trim": [_i32],
    "comms_buf_record_ready": [_vp, _vp],
    "comms_buf_wait_ready": [_vp, _vp],
    "comms_buf_record_use": [_vp, _vp],
    "comms_buf_sync": [_vp],
    "comms_stream_create": [_i32, _pp],
    "comms_stream_synchronize": [_i32, _vp],
    "comms_stream_destroy": [_i32, _vp],
    "comms_stream_pool_trim": [_i32],
    "comms_timer_create": [_sz, _i32, _pp],
    "comms_timer_create_stamps": [_sz, _i32, _pp],
    "comms_timer_add_stamps": [_vp, _sz],
    "comms_timer_set_stride": [_vp, _sz],
    "comms_timer_read_stamps": [_vp, _vp, _sz, _psz],
    "comms_timer_reset": [_vp],
    "comms_timer_read": [_vp, _vp, _sz, _psz],
    "comms_timer_destroy": [_vp],
    "comms_fir_set_timer": [_vp, _vp],
    "comms_fir_set_input_format": [_vp, _i32, C.c_float],
    "comms_chain_set_input_format": [_vp, _i32, C.c_float],
    "comms_chain_set_output_format": [_vp, _i32, _i32, _vp],
    "comms_mixer_set_timer": [_vp, _vp],
    "comms_pulse_set_timer": [_vp, _vp],
    "comms_fmdemod_set_timer": [_vp, _vp],
    "comms_fft_set_timer": [_vp, _vp],
    "comms_chain_set_timer": [_vp, _vp],
    "comms_fir_create": [_vp, _sz, _vp, _sz, _i32, _pp],
    "comms_fir_set_algo": [_vp, _i32],
    "comms_fir_get_algo": [_vp, _sz, C.POINTER(_i32)],
    "comms_fir_get_kernel": [_vp, _sz, C.c_char_p, _sz],
    "comms_fir_run": [_vp, _vp, _sz, _vp],
    "comms_fir_run_dev": [_vp, _vp, _sz, _vp, _vp],
    "comms_fir_get_state": [_vp, _vp, _sz],
    "comms_fir_set_state": [_vp, _vp, _sz],
    "comms_fir_destroy": [_vp],
    "comms_fir_i16_create": [_vp, _sz, _vp, _sz, _i32, _pp],
    "comms_fir_i16_run": [_vp, _vp, _sz, _vp],
    "comms_fir_i16_run_dev": [_vp, _vp, _sz, _vp, _vp],
    "comms_fir_i16_get_state": [_vp, _vp, _sz],
    "comms_fir_i16_destroy": [_vp],
    "comms_fir_f64_create": [_vp, _sz, _vp, _sz, _i32, _pp],
    "comms_fir_f64_run": [_vp, _vp, _sz, _vp],
    "comms_fir_f64_run_dev": [_vp, _vp, _sz, _vp, _vp],
    "comms_fir_f64_get_state": [_vp, _vp, _sz],
    "comms_fir_f64_set_state": [_vp, _vp, _sz],
    "comms_fir_f64_destroy": [_vp],
    "comms_pulse_f64_create": [_vp, _sz, _sz, _i32, _pp],
    "comms_pulse_f64_run": [_vp, _vp, _sz, _vp],
    "comms_pulse_f64_run_dev": [_vp, _vp, _sz, _vp, _vp],
    "comms_pulse_f64_destroy": [_vp],
    "comms_pulse_i16_create": [_vp, _sz, _sz, _i32, _pp],
    "comms_pulse_i16_run": [_vp, _vp, _sz, _vp],
    "comms_pulse_i16_run_dev": [_vp, _vp, _sz, _vp, _vp],
    "comms_pulse_i16_destroy": [_vp],
    "comms_pulse_create": [_vp, _sz, _sz, _i32, _pp],
    "comms_pulse_run": [_vp, _vp, _sz, _vp],
    "comms_pulse_run_dev": [_vp, _vp, _sz, _vp, _vp],
    "comms_pulse_set_mixer": [_vp, _f64, _f64],
    "comms_pulse_get_phase": [_vp, C.POINTER(_f64)],
    "comms_pulse_set_output_format": [_vp, _i32, C.c_float],
    "comms_pulse_set_input_format": [_vp, _i32, _i32, _vp],
    "comms_pulse_destroy": [_vp],
    "comms_mixer_create": [_f64, _f64, _i32, _pp],
    "comms_mixer_run": [_vp, _vp, _sz, _vp],
    "comms_mixer_run_dev": [_vp, _vp, _sz, _vp, _vp],
    "comms_mixer_run_f64": [_vp, _vp, _sz, _vp],
    "comms_mixer_run_f64_dev": [_vp, _vp, _sz, _vp, _vp],
    "comms_mixer_get_phase": [_vp, C.POINTER(_f64)],
    "comms_mixer_set_phase": [_vp, _f64],
    "comms_mixer_destroy": [_vp],
    "comms_decimate_out_len": [_sz, _sz, _psz],
    "comms_upsample_out_len": [_sz, _sz, _psz],
    "comms_decimate_run": [_vp, _sz, _sz, _sz, _vp, _psz, _i32],
    "comms_decimate_run_dev": [_vp, _sz, _sz, _sz, _vp, _psz, _i32, _vp],
    "comms_upsample_run": [_vp, _sz, _sz, _sz, _vp, _psz, _i32],
    "comms_upsample_run_dev": [_vp, _sz, _sz, _sz, _vp, _psz, _i32, _vp],
    "comms_fmdemod_create": [_i32, _pp],
    "comms_fmdemod_run": [_vp, _vp, _sz, _vp],
    "comms_fmdemod_run_dev": [_vp, _vp, _sz, _vp, _vp],
    "comms_fmdemod_get_prev": [_vp, _vp],
    "comms_fmdemod_set_prev": [_vp, _vp],
    "comms_fmdemod_destroy": [_vp],
    "comms_fft_create": [_sz, _i32, _i32, _pp],
    "comms_fft_run": [_vp, _vp, _sz, _vp],
    "comms_fft_run_dev": [_vp, _vp, _sz, _vp, _vp],
    "comms_fft_destroy": [_vp],
    "comms_fft_f64_create": [_sz, _i32, _i32, _pp],
    "comms_fft_f64_run": [_vp, _vp, _sz, _vp],
    "comms_fft_f64_run_dev": [_vp, _vp, _sz, _vp, _vp],
    "comms_fft_f64_destroy": [_vp],
    "comms_fmdemod_f64_create": [_i32, _pp],
    "comms_fmdemod_f64_run": [_vp, _vp, _sz, _vp],
    "comms_fmdemod_f64_run_dev": [_vp, _vp, _sz, _vp, _vp],
    "comms_fmdemod_f64_get_prev": [_vp, _vp],
    "comms_fmdemod_f64_set_prev": [_vp, _vp],
    "comms_fmdemod_f64_destroy": [_vp],
    "comms_rrc_taps": [_u32, _f64, _f64, _vp],
    "comms_rc_taps": [_u32, _f64, _f64, _vp],
    "comms_gaussian_taps": [_u32, _f64, _f64, _vp],
    "comms_rect_taps": [_sz, _vp],
    "comms_chain_create": [_f64, _f64, _vp, _sz, _sz, _i32, _i32, _pp],
    "comms_chain_create_ex": [_f64, _f64, _vp, _sz, _sz, _i32, _i32, _pp],
    "comms_chain_is_fused": [_vp, C.POINTER(_i32)],
    "comms_chain_run_dev": [_vp, _vp, _sz, _vp, _vp],
    "comms_chain_run": [_vp, _vp, _sz, _vp],
    "comms_chain_set_fir_state": [_vp, _vp, _sz],
    "comms_chain_get_fir_state": [_vp, _vp, _sz],
    "comms_chain_get_phase": [_vp, C.POINTER(_f64)],
    "comms_chain_set_phase": [_vp, _f64],
    "comms_chain_get_fm_prev": [_vp, _vp],
    "comms_chain_set_fm_prev": [_vp, _vp],
    "comms_chain_destroy": [_vp],
    "comms_iq_i16_to_c32": [_vp, _sz, C.c_float, _vp, _i32],
    "comms_iq_c32_to_i16": [_vp, _sz, C.c_float, _vp, _i32],
    "comms_iq_u8_to_c32": [_vp, _sz, _vp, _i32],
    "comms_iq_i16_to_c32_dev": [_vp, _sz, C.c_float, _vp, _i32, _vp],
    "comms_iq_c32_to_i16_dev": [_vp, _sz, C.c_float, _vp, _i32, _vp],
    "comms_iq_u8_to_c32_dev": [_vp, _sz, _vp, _i32, _vp],
    "comms_iq_real_to_c32_dev": [_vp, _sz, _vp, _i32, _vp],
    "comms_iq_c32_re_dev": [_vp, _sz, _vp, _i32, _vp],
    "comms_rfir_create": [_vp, _sz, _vp, _sz, _sz, _i32, _pp],
    "comms_rfir_out_len": [_sz, _sz, _psz],
    "comms_rfir_run_dev": [_vp, _vp, _sz, _vp, _vp],
    "comms_rfir_run": [_vp, _vp, _sz, _vp],
    "comms_rfir_get_state": [_vp, _vp, _sz],
    "comms_rfir_set_state": [_vp, _vp, _sz],
    "comms_rfir_get_kernel": [_vp, _sz, C.c_char_p, _sz],
    "comms_rfir_set_timer": [_vp, _vp],
    "comms_rfir_destroy": [_vp],
    "comms_resample_create": [_vp, _sz, _sz, _sz, _i32, _i32, _pp],
    "comms_resample_out_len": [_sz, _sz, _sz, _psz],
    "comms_resample_state_len": [_sz, _sz, _psz],
    "comms_resample_run_dev": [_vp, _vp, _sz, _vp, _vp],
    "comms_resample_run": [_vp, _vp, _sz, _vp],
    "comms_resample_get_state": [_vp, _vp, _sz],
    "comms_resample_set_state": [_vp, _vp, _sz],
    "comms_resample_get_kernel": [_vp, _sz, C.c_char_p, _sz],
    "comms_resample_set_timer": [_vp, _vp],
    "comms_resample_destroy": [_vp],
    "comms_channelizer_create": [_vp, _sz, _sz, _sz, _i32, _i32, _pp],
    "comms_channelizer_out_len": [_sz, _sz, _psz],
    "comms_channelizer_state_len": [_sz, _psz],
    "comms_channelizer_run_dev": [_vp, _vp, _sz, _vp, _vp],
    "comms_channelizer_run": [_vp, _vp, _sz, _vp],
    "comms_channelizer_get_state": [_vp, _vp, _sz],
    "comms_channelizer_set_state": [_vp, _vp, _sz],
    "comms_channelizer_get_phase": [_vp, C.POINTER(_u64)],
    "comms_channelizer_set_phase": [_vp, _u64],
    "comms_channelizer_get_kernel": [_vp, _sz, C.c_char_p, _sz],
    "comms_channelizer_set_timer": [_vp, _vp],
    "comms_channelizer_destroy": [_vp],
    "comms_symsync_create": [_vp, _sz, _sz, _sz, _i32, _pp],
    "comms_symsync_out_len": [_sz, _sz, _psz],
    "comms_symsync_state_len": [_sz, _sz, _psz],
    "comms_symsync_set_timing": [_vp, _f64],
    "comms_symsync_get_timing": [_vp, C.POINTER(_u32)],
    "comms_symsync_set_rotation": [_vp, _f64, _f64],
    "comms_symsync_get_phase": [_vp, C.POINTER(_f64)],
    "comms_symsync_set_output_format": [_vp, _i32, _i32, _vp],
    "comms_symsync_run_dev": [_vp, _vp, _sz, _vp, _vp],
    "comms_symsync_run": [_vp, _vp, _sz, _vp],
    "comms_symsync_get_state": [_vp, _vp, _sz],
    "comms_symsync_set_state": [_vp, _vp, _sz],
    "comms_symsync_get_kernel": [_vp, _sz, C.c_char_p, _sz],
    "comms_symsync_set_timer": [_vp, _vp],
    "comms_symsync_destroy": [_vp],
    "comms_bpsk_byte_mod": [_vp, _sz, _vp, _i32],
    "comms_qpsk_byte_mod": [_vp, _sz, _vp, _i32],
    "comms_bpsk_bit_mod": [_vp, _sz, _vp, _i32],
    "comms_qpsk_bit_mod": [_vp, _sz, _vp, _i32],
    "comms_bpsk_byte_mod_dev": [_vp, _sz, _vp, _i32, _vp],
    "comms_qpsk_byte_mod_dev": [_vp, _sz, _vp, _i32, _vp],
    "comms_bpsk_bit_mod_dev": [_vp, _sz, _vp, _i32, _vp],
    "comms_qpsk_bit_mod_dev": [_vp, _sz, _vp, _i32, _vp],
    "comms_sym_to_bits": [_vp, _sz, _i32, _vp, _vp, _i32],
    "comms_sym_to_bits_dev": [_vp, _sz, _i32, _vp, _vp, _i32, _vp],
    "comms_bit_errors": [_vp, _vp, _u64, C.POINTER(_u64), _i32],
    "comms_bit_errors_dev": [_vp, _vp, _u64, C.POINTER(_u64), _i32, _vp],
    "comms_prns_create": [_u64, _u64, _i32, _i32, _pp],
    "comms_prns_run": [_vp, _sz, _i32, _vp],
    "comms_prns_run_dev": [_vp, _sz, _i32, _vp, _vp],
    "comms_prns_get_state": [_vp, C.POINTER(_u64)],
    "comms_prns_set_state": [_vp, _u64],
    "comms_prns_skip": [_vp, _u64],
    "comms_prns_set_timer": [_vp, _vp],
    "comms_prns_destroy": [_vp],
    "comms_noise_create": [_u64, _u64, _i32, _pp],
    "comms_noise_get_pos": [_vp, C.POINTER(_u64)],
    "comms_noise_set_pos": [_vp, _u64],
    "comms_noise_skip": [_vp, _u64],
    "comms_noise_bits_run": [_vp, _sz, _i32, _vp],
    "comms_noise_bits_run_dev": [_vp, _sz, _i32, _vp, _vp],
    "comms_noise_uniform_run": [_vp, _sz, C.c_float, C.c_float, _vp],
    "comms_noise_uniform_run_dev": [_vp, _sz, C.c_float, C.c_float, _vp, _vp],
    "comms_noise_normal_run": [_vp, _sz, _f64, _f64, _vp],
    "comms_noise_normal_run_dev": [_vp, _sz, _f64, _f64, _vp, _vp],
    "comms_noise_normal_f64_run": [_vp, _sz, _f64, _f64, _vp],
    "comms_noise_normal_f64_run_dev": [_vp, _sz, _f64, _f64, _vp, _vp],
    "comms_awgn_run": [_vp, _vp, _sz, C.c_float, _vp],
    "comms_awgn_run_dev": [_vp, _vp, _sz, C.c_float, _vp, _vp],
    "comms_awgn_set_input_format": [_vp, _i32, C.c_float],
    "comms_noise_set_timer": [_vp, _vp],
    "comms_noise_destroy": [_vp],
    "comms_frequency_offset_estimate": [_vp, _sz, C.POINTER(_f64), _i32],
    "comms_psk_phase_estimate": [_vp, _sz, _u32, C.POINTER(_f64), _i32],
    "comms_qam_phase_estimate": [_vp, _sz, C.POINTER(_f64), _i32],
    "comms_frequency_offset_estimate_dev": [_vp, _sz, C.POINTER(_f64), _i32, _vp],
    "comms_psk_phase_estimate_dev": [_vp, _sz, _u32, C.POINTER(_f64), _i32, _vp],
    "comms_qam_phase_estimate_dev": [_vp, _sz, C.POINTER(_f64), _i32, _vp],
    "comms_timing_create": [_u32, _u32, _f64, _i32, _pp],
    "comms_timing_push": [_vp, _vp, _sz, C.POINTER(_f64)],
    "comms_timing_push_dev": [_vp, _vp, _sz, C.POINTER(_f64), _vp],
    "comms_timing_get_kernel": [_vp, _sz, C.c_char_p, _sz],
    "comms_timing_destroy": [_vp],
    "comms_qfilt_taps": [_u32, _f64, _u32, _vp],
    "comms_syncest_create": [_u32, _u32, _f64, _i32, _pp],
    "comms_syncest_run_dev": [_vp, _vp, _sz, _vp, _vp],
    "comms_syncest_run": [_vp, _vp, _sz, _vp],
    "comms_syncest_get_kernel": [_vp, _sz, C.c_char_p, _sz],
    "comms_syncest_set_timer": [_vp, _vp],
    "comms_syncest_destroy": [_vp],
    "comms_psk_phase_estimate_c32": [_vp, _sz, _u32, C.POINTER(_f64), _i32],
    "comms_qam_phase_estimate_c32": [_vp, _sz, C.POINTER(_f64), _i32],
    "comms_psk_phase_estimate_c32_dev": [_vp, _sz, _u32, C.POINTER(_f64), _i32, _vp],
    "comms_qam_phase_estimate_c32_dev": [_vp, _sz, C.POINTER(_f64), _i32, _vp],
    "comms_framesync_create": [_vp, _sz, _f64, _sz, _i32, _pp],
    "comms_framesync_run_dev": [_vp, _vp, _sz, _vp, _sz, _psz, _vp],
    "comms_framesync_run": [_vp, _vp, _sz, _vp, _sz, _psz],
    "comms_framesync_flush": [_vp, _vp, _sz, _psz],
    "comms_framesync_state_len": [_sz, _sz, _psz],
    "comms_framesync_get_state": [_vp, _vp, _sz],
    "comms_framesync_set_state": [_vp, _vp, _sz],
    "comms_framesync_get_position": [_vp, C.POINTER(_u64)],
    "comms_framesync_set_position": [_vp, _u64],
    "comms_framesync_set_threshold": [_vp, _f64],
    "comms_framesync_get_kernel": [_vp, _sz, C.c_char_p, _sz],
    "comms_framesync_set_timer": [_vp, _vp],
    "comms_framesync_destroy": [_vp],
    "comms_deframe_create": [_sz, _sz, _sz, _i32, _vp, _i32, _i32, _pp],
    "comms_deframe_set_word_energy": [_vp, _f64],
    "comms_deframe_set_output_format": [_vp, _i32],
    "comms_deframe_set_llr_scale": [_vp, C.c_float],
    "comms_deframe_frames_ready": [_vp, _sz, _vp, _sz, _psz],
    "comms_deframe_run_dev": [_vp, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _psz, _vp],
    "comms_deframe_run": [_vp, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _psz],
    "comms_deframe_flush": [_vp, _psz],
    "comms_deframe_state_len": [_sz, _sz, _psz],
    "comms_deframe_get_state": [_vp, _vp, _sz],
    "comms_deframe_set_state": [_vp, _vp, _sz],
    "comms_deframe_get_position": [_vp, C.POINTER(_u64)],
    "comms_deframe_set_position": [_vp, _u64],
    "comms_deframe_get_pending": [_vp, _vp, _sz, _psz],
    "comms_deframe_set_pending": [_vp, _vp, _sz],
    "comms_deframe_get_kernel": [_vp, _sz, C.c_char_p, _sz],
    "comms_deframe_set_timer": [_vp, _vp],
    "comms_deframe_destroy": [_vp],
    "comms_convenc_create": [_i32, _i32, _vp, _i32, _sz, _i32, _pp],
    "comms_convenc_run_dev": [_vp, _vp, _sz, _vp, _vp],
    "comms_convenc_run": [_vp, _vp, _sz, _vp],
    "comms_convenc_get_kernel": [_vp, _sz, C.c_char_p, _sz],
    "comms_convenc_set_timer": [_vp, _vp],
    "comms_convenc_destroy": [_vp],
    "comms_viterbi_create": [_i32, _i32, _vp, _i32, _sz, _sz, _i32, _pp],
    "comms_viterbi_set_quant_scale": [_vp, C.c_float],
    "comms_viterbi_run_dev": [_vp, _vp, _sz, _vp, _vp, _vp],
    "comms_viterbi_run": [_vp, _vp, _sz, _vp, _vp],
    "comms_viterbi_get_kernel": [_vp, _sz, C.c_char_p, _sz],
    "comms_viterbi_set_timer": [_vp, _vp],
    "comms_viterbi_destroy": [_vp],
    "comms_ldpcenc_create": [_i32, _i32, _i32, _vp, _i32, _pp],
    "comms_ldpcenc_run_dev": [_vp, _vp, _sz, _vp, _vp],
    "comms_ldpcenc_run": [_vp, _vp, _sz, _vp],
    "comms_ldpcenc_get_kernel": [_vp, _sz, C.c_char_p, _sz],
    "comms_ldpcenc_set_timer": [_vp, _vp],
    "comms_ldpcenc_destroy": [_vp],
    "comms_ldpcdec_create": [_i32, _i32, _i32, _vp, _i32, _i32, _sz, _i32, _pp],
    "comms_ldpcdec_set_quant_scale": [_vp, C.c_float],
    "comms_ldpcdec_run_dev": [_vp, _vp, _sz, _vp, _vp, _vp],
    "comms_ldpcdec_run": [_vp, _vp, _sz, _vp, _vp],
    "comms_ldpcdec_get_kernel": [_vp, _sz, C.c_char_p, _sz],
    "comms_ldpcdec_set_timer": [_vp, _vp],
    "comms_ldpcdec_destroy": [_vp],
    "comms_ratematch_create": [_sz, _vp, _sz, _sz, _vp, _vp, _sz, _i32, _pp],
    "comms_ratematch_get_map": [_vp, _vp, _sz],
    "comms_ratematch_tx_run_dev": [_vp, _vp, _sz, _vp, _vp],
    "comms_ratematch_rx_run_dev": [_vp, _vp, _sz, _vp, _vp],
    "comms_ratematch_tx_run": [_vp, _vp, _sz, _vp],
    "comms_ratematch_rx_run": [_vp, _vp, _sz, _vp],
    "comms_ratematch_get_kernel": [_vp, _i32, _sz, C.c_char_p, _sz],
    "comms_ratematch_set_timer": [_vp, _vp],
    "comms_ratematch_destroy": [_vp],
    "comms_crc_create": [_i32, _u32, _u32, _u32, _sz, _i32, _pp],
    "comms_crc_attach_run_dev": [_vp, _vp, _sz, _vp, _vp],
    "comms_crc_check_run_dev": [_vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp],
    "comms_crc_attach_run": [_vp, _vp, _sz, _vp],
    "comms_crc_check_run": [_vp, _vp, _sz, _vp, _vp, _vp, _psz],
    "comms_crc_get_kernel": [_vp, _i32, _sz, C.c_char_p, _sz],
    "comms_crc_set_timer": [_vp, _vp],
    "comms_crc_destroy": [_vp],
    "comms_constellation_qam": [_i32, _f64, _vp],
    "comms_constellation_psk": [_i32, _f64, _vp],
    "comms_symmap_create": [_i32, _vp, _sz, _vp, _sz, _sz, _i32, _pp],
    "comms_symmap_run_dev": [_vp, _vp, _sz, _vp, _vp],
    "comms_symmap_run": [_vp, _vp, _sz, _vp],
    "comms_symmap_get_kernel": [_vp, _sz, C.c_char_p, _sz],
    "comms_symmap_set_timer": [_vp, _vp],
    "comms_symmap_destroy": [_vp],
    "comms_demap_create": [_i32, _vp, _sz, _i32, _i32, _pp],
    "comms_demap_set_output_format": [_vp, _i32],
    "comms_demap_set_llr_scale": [_vp, C.c_float],
    "comms_demap_run_dev": [_vp, _vp, _sz, _vp, _vp],
    "comms_demap_run": [_vp, _vp, _sz, _vp],
    "comms_demap_run_weighted_dev": [_vp, _vp, _vp, _sz, _sz, _vp, _vp],
    "comms_demap_run_weighted": [_vp, _vp, _vp, _sz, _sz, _vp],
    "comms_demap_get_kernel": [_vp, _sz, C.c_char_p, _sz],
    "comms_demap_set_timer": [_vp, _vp],
    "comms_demap_destroy": [_vp],
    "comms_ofdm_create": [_i32, _i32, _vp, _vp, _vp, _sz, _vp, _sz, _sz, _i32, _i32, _pp],
    "comms_ofdm_set_scale": [_vp, C.c_float],
    "comms_ofdm_mod_run_dev": [_vp, _vp, _sz, _vp, _vp],
    "comms_ofdm_mod_run": [_vp, _vp, _sz, _vp],
    "comms_ofdm_demod_run_dev": [_vp, _vp, _sz, _vp, _vp],
    "comms_ofdm_demod_run": [_vp, _vp, _sz, _vp],
    "comms_ofdm_demod_csi_run_dev": [_vp, _vp, _sz, _vp, _vp, _vp],
    "comms_ofdm_demod_csi_run": [_vp, _vp, _sz, _vp, _vp],
    "comms_ofdm_get_kernel": [_vp, _i32, _sz, C.c_char_p, _sz],
    "comms_ofdm_set_timer": [_vp, _vp],
    "comms_ofdm_destroy": [_vp],
    "comms_ofdmsync_create": [_sz, _sz, _f64, _sz, _sz, _sz, _i32, _pp],
    "comms_ofdmsync_run_dev": [_vp, _vp, _sz, _vp, _vp, _sz, _psz, _vp],
    "comms_ofdmsync_run": [_vp, _vp, _sz, _vp, _vp, _sz, _psz],
    "comms_ofdmsync_flush": [_vp, _vp, _vp, _sz, _psz],
    "comms_ofdmsync_correct_run_dev": [_vp, _vp, _sz, _vp, _vp, _vp],
    "comms_ofdmsync_correct_run": [_vp, _vp, _sz, _vp, _vp],
    "comms_ofdmsync_state_len": [_sz, _sz, _sz, _psz],
    "comms_ofdmsync_get_state": [_vp, _vp, _sz],
    "comms_ofdmsync_set_state": [_vp, _vp, _sz],
    "comms_ofdmsync_get_position": [_vp, C.POINTER(_u64)],
    "comms_ofdmsync_set_position": [_vp, _u64],
    "comms_ofdmsync_set_threshold": [_vp, _f64],
    "comms_ofdmsync_get_kernel": [_vp, _sz, C.c_char_p, _sz],
    "comms_ofdmsync_set_timer": [_vp, _vp],
    "comms_ofdmsync_destroy": [_vp],
    "comms_window_taps": [_i32, _sz, _vp],
    "comms_spectrum_create": [_i32, _vp, _sz, _sz, C.c_float, _i32, _i32, _pp],
    "comms_spectrum_out_len": [_vp, _sz, _psz],
    "comms_spectrum_state_len": [_i32, _psz],
    "comms_spectrum_run_dev": [_vp, _vp, _sz, _vp, _vp],
    "comms_spectrum_run": [_vp, _vp, _sz, _vp],
    "comms_spectrum_get_state": [_vp, _vp, _sz],
    "comms_spectrum_set_state": [_vp, _vp, _sz],
    "comms_spectrum_get_position": [_vp, C.POINTER(_u64)],
    "comms_spectrum_set_position": [_vp, _u64],
    "comms_spectrum_get_acc": [_vp, _vp, _sz],
    "comms_spectrum_set_acc": [_vp, _vp, _sz],
    "comms_spectrum_get_kernel": [_vp, _sz, C.c_char_p, _sz],
    "comms_spectrum_set_timer": [_vp, _vp],
    "comms_spectrum_destroy": [_vp],
    "comms_nco_create": [_f64, _f64, _i32, _pp],
    "comms_nco_run": [_vp, _vp, _sz, _vp],
    "comms_nco_run_dev": [_vp, _vp, _sz, _vp, _vp],
    "comms_nco_get_phase": [_vp, C.POINTER(_f64)],
    "comms_nco_get_kernel": [_vp, _sz, C.c_char_p, _sz],
    "comms_nco_destroy": [_vp],
    "comms_synth_iq_dev": [_vp, _sz, _u64, _u64, _i32, _vp],
    "comms_shard_range": [_sz, _u32, _u32, _psz, _psz],
    "comms_state_from_halo": [_vp, _sz, _vp],
    "comms_shard_mixer_phase": [_f64, _f64, C.c_int64, C.POINTER(_f64)],
    "comms_chain_prefix_len": [_sz, _sz, _i32, _psz],
}
_OTHER = {
    "comms_version": (C.c_char_p, []),
    "comms_last_error": (C.c_char_p, []),
    "comms_buf_ptr": (_vp, [_vp]),
    "comms_buf_size": (_sz, [_vp]),
    "comms_qfilt_len": (_sz, [_u32]),
    "comms_deframe_frame_bytes": (_sz, [_vp]),
    "comms_convenc_in_frame_bytes": (_sz, [_vp]),
    "comms_convenc_out_frame_bytes": (_sz, [_vp]),
    "comms_viterbi_in_frame_bytes": (_sz, [_vp]),
    "comms_viterbi_out_frame_bytes": (_sz, [_vp]),
    "comms_ldpcenc_in_frame_bytes": (_sz, [_vp]),
    "comms_ldpcenc_out_frame_bytes": (_sz, [_vp]),
    "comms_ldpcdec_in_frame_bytes": (_sz, [_vp]),
    "comms_ldpcdec_out_frame_bytes": (_sz, [_vp]),
    "comms_ratematch_n_tx_bits": (_sz, [_vp]),
    "comms_ratematch_tx_in_frame_bytes": (_sz, [_vp]),
    "comms_ratematch_tx_out_frame_bytes": (_sz, [_vp]),
    "comms_ratematch_rx_in_frame_bytes": (_sz, [_vp]),
    "comms_ratematch_rx_out_frame_bytes": (_sz, [_vp]),
    "comms_crc_payload_frame_bytes": (_sz, [_vp]),
    "comms_crc_coded_frame_bytes": (_sz, [_vp]),
    "comms_symmap_in_frame_bytes": (_sz, [_vp]),
    "comms_symmap_out_frame_syms": (_sz, [_vp]),
    "comms_demap_in_frame_bytes": (_sz, [_vp]),
    "comms_demap_out_frame_bytes": (_sz, [_vp]),
    "comms_ofdm_data_syms": (_sz, [_vp]),
    "comms_ofdm_frame_samples": (_sz, [_vp]),
    "comms_buf_device": (_i32, [_vp]),
    "comms_synth_iq_host": (None, [_vp, _sz, _u64, _u64]),
}


def all_symbols():
    return sorted(list(_PROTOS) + list(_OTHER))


def lib():
    """The loaded library (raises if it has not been built -- no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "%s not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc, gfx950).  comms_rs_amd has no CPU fallback." % LIB_PATH)
        # PyTorch bundles its own HIP runtime.  When both live in one process the
        # runtime torch ships must be the one that is loaded first, or torch
        # cannot see the GPU afterwards -- so let torch load it if torch is here.
        if os.environ.get("COMMS_NO_TORCH_PRELOAD") != "1":
            try:
                import torch  # noqa: F401
            except Exception:
                pass
        l = C.CDLL(LIB_PATH)
        missing = [n for n in all_symbols() if not hasattr(l, n)]
        if missing:
            raise ImportError("%s lacks symbols declared in include/comms_hip.h: %s"
                              % (LIB_PATH, ", ".join(missing)))
        for name, args in _PROTOS.items():
            f = getattr(l, name)
            f.restype = _i32
            f.argtypes = args
        for name, (res, args) in _OTHER.items():
            f = getattr(l, name)
            f.restype = res
            f.argtypes = args
        _lib = l
    return _lib


def check(status):
    if status != COMMS_OK:
        raise CommsError(status, lib().comms_last_error().decode("utf-8", "replace"))
