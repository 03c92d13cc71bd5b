"""ctypes binding of libssrhip.so (the C ABI declared in include/ssr_hip.h).

The library is built in-tree by ``ssr_eval_amd.build.build()`` (``hipcc --offload-arch=gfx950``).
There is NO fallback: if the shared object is missing or no HIP device is present every entry
point raises.  Nothing here imports ``oracle``.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libssrhip.so")

SSR_F32, SSR_F64 = 0, 1
M_LSD, M_LOG_SISPEC, M_SISPEC, M_SSIM, M_ALL = 1, 2, 4, 8, 15
STFT_MAG, STFT_COMPLEX = 1, 2
LOWPASS_SEGMENTS, LOWPASS_FUSED, LOWPASS_CONV = 0, 1, 2
PAD_REFLECT, PAD_CONSTANT = 0, 1
ERR_INVALID_ARG, ERR_UNSUPPORTED, ERR_HIP, ERR_WORKSPACE = -1, -2, -3, -4      # include/ssr_hip.h
MAX_BANDS = 8                                                                   # SSR_MAX_BANDS
STOI, ESTOI, STOI_BOTH = 1, 2, 3                                                # SSR_STOI, SSR_ESTOI, SSR_STOI_BOTH
WAVE_SNR, WAVE_SI_SDR, WAVE_SEG_SNR = 1, 2, 4                                   # SSR_WAVE_SNR, SSR_WAVE_SI_SDR, SSR_WAVE_SEG_SNR
MEL_LSD, MEL_L1, MEL_MCD, MEL_MAX = 1, 2, 4, 256                                # SSR_MEL_LSD, SSR_MEL_L1, SSR_MEL_MCD, SSR_MEL_MAX
DTW_MAX_RADIUS = 31                                                             # SSR_DTW_MAX_RADIUS
QUAL_LLR, QUAL_CEP, QUAL_WSS, QUAL_FWSEG = 1, 2, 4, 8                           # SSR_QUAL_LLR, SSR_QUAL_CEP, SSR_QUAL_WSS, SSR_QUAL_FWSEG
PITCH_F0_RMSE, PITCH_F0_CORR, PITCH_GPE, PITCH_VDE, PITCH_FFE = 1, 2, 4, 8, 16  # SSR_PITCH_*
PHASE_IP, PHASE_GD, PHASE_IAF = 1, 2, 4                                         # SSR_PHASE_IP, SSR_PHASE_GD, SSR_PHASE_IAF
MRSTFT_MAX_RES = 8                                                              # SSR_MRSTFT_MAX_RES
BSS_MAX_TAPS = 512                                                              # SSR_BSS_MAX_TAPS
BOOTSTRAP_UTTERANCE, BOOTSTRAP_SPEAKER, BOOTSTRAP_MAX_Q = 0, 1, 8                # SSR_BOOTSTRAP_*
SPECTRUM_MAX_BANDS = 40                                                         # SSR_SPECTRUM_MAX_BANDS
AUDITORY_MIN_BANDS, AUDITORY_MAX_BANDS, AUDITORY_MAX_BLOCKS = 3, 64, 65536      # SSR_AUDITORY_MIN_BANDS, _MAX_BANDS, _MAX_BLOCKS
MODULATION_BANDS, MODULATION_MAX_BLOCKS = 8, 65536                              # SSR_MODULATION_BANDS, SSR_MODULATION_MAX_BLOCKS
DISTRIBUTION_MAX_DIM, DISTRIBUTION_MAX_GAMMA, DISTRIBUTION_MAX_PAIR_ROWS = 1024, 8, 2048   # SSR_DISTRIBUTION_MAX_DIM, _MAX_GAMMA, _MAX_PAIR_ROWS
DISTRIBUTION_PAIRWISE_WORKSPACE = 16640                                         # SSR_DISTRIBUTION_PAIRWISE_WORKSPACE
CSII_BANDS, CSII_COLUMNS = 21, 13                                               # SSR_CSII_BANDS, SSR_CSII_COLUMNS
ALIGN_MAX_LAG, ALIGN_COLUMNS = 4096, 4                                          # SSR_ALIGN_MAX_LAG, SSR_ALIGN_COLUMNS
NMR_BANDS, NMR_COLUMNS, NMR_TABLE = 128, 6, 8                                   # SSR_NMR_BANDS, SSR_NMR_COLUMNS, SSR_NMR_TABLE

_vp, _i, _i64, _sz, _u = C.c_void_p, C.c_int, C.c_int64, C.c_size_t, C.c_uint

# name -> (restype, argtypes): exactly the symbols include/ssr_hip.h declares
SIGNATURES = {
    "ssr_last_error": (C.c_char_p, []),
    "ssr_version": (_i, []),
    "ssr_plan_create": (_i, [_i, _i, _i, C.POINTER(_vp)]),
    "ssr_plan_create_ex": (_i, [_i, _i, _vp, _i, _i, C.POINTER(_vp)]),
    "ssr_plan_destroy": (_i, [_vp]),
    "ssr_plan_query": (_i, [_vp] + [C.POINTER(_i)] * 6),
    "ssr_plan_set_lowpass_engine": (_i, [_vp, _i]),
    "ssr_plan_set_tl_weights": (_i, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "ssr_tl_weights": (_i, [_i, _vp, _vp, _vp, _vp, _vp]),
    "ssr_tl_weights_ex": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ssr_num_frames": (_i64, [_vp, _i64]),
    "ssr_stft": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "ssr_magphase": (_i, [_vp, _vp, _i64, C.c_float, _vp, _vp, _vp, _vp]),
    "ssr_pair_metrics_workspace_bytes": (_sz, [_vp, _i, _i, _i64]),
    "ssr_pair_metrics_workspace_bytes_for": (_sz, [_vp, _i, _i, _i64, _u]),
    "ssr_pair_metrics": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i64, _u, _vp, _vp, _sz, _vp]),
    "ssr_pair_metrics_multi_workspace_bytes": (_sz, [_vp, _i, _i, _i, _i64, _u]),
    "ssr_pair_metrics_multi": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i64, _u, _vp, _vp, _sz, _vp]),
    "ssr_pair_metrics_multi_est64_workspace_bytes": (_sz, [_vp, _i, _i, _i, _i64, _u]),
    "ssr_pair_metrics_multi_est64": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i64, _u, _vp, _vp, _sz, _vp]),
    "ssr_pair_metrics_est64": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i64, _u, _vp, _vp, _sz, _vp]),
    "ssr_pair_metrics_f64": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i64, _u, _vp, _vp, _sz, _vp]),
    "ssr_pair_metrics_stages": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i64, _u, _vp, _vp, _sz, _vp, _i]),
    "ssr_spectrogram_metrics_workspace_bytes": (_sz, [_i, _i, _i]),
    "ssr_spectrogram_metrics": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _u, _vp, _vp, _sz, _vp]),
    "ssr_spectrogram_lsd_bands_workspace_bytes": (_sz, [_i, _i, _i]),
    "ssr_spectrogram_lsd_bands": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _i, _vp, _vp, _sz, _vp]),
    "ssr_pair_lsd_bands_workspace_bytes": (_sz, [_vp, _i, _i, _i, _i64, _i]),
    "ssr_pair_lsd_bands": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i64, _vp, _i, _vp, _vp, _sz, _vp]),
    "ssr_pair_lsd_bands_est64": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i64, _vp, _i, _vp, _vp, _sz, _vp]),
    "ssr_spectrogram_mel_workspace_bytes": (_sz, [_i, _i]),
    "ssr_spectrogram_mel": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _i, _vp, _vp, _sz, _vp]),
    "ssr_spectrogram_mel_metrics_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "ssr_spectrogram_mel_metrics": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "ssr_pair_mel_metrics_workspace_bytes": (_sz, [_vp, _i, _i, _i, _i64, _i, _i]),
    "ssr_pair_mel_metrics": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i64, _vp, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "ssr_pair_mel_metrics_est64": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i64, _vp, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "ssr_spectrogram_mel_dtw_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i]),
    "ssr_spectrogram_mel_dtw": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "ssr_pair_mel_dtw_workspace_bytes": (_sz, [_vp, _i, _i, _i, _i64, _i, _i, _i]),
    "ssr_pair_mel_dtw": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i64, _vp, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "ssr_pair_mel_dtw_est64": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i64, _vp, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "ssr_stoi_workspace_bytes": (_sz, [_vp, _i, _vp, _i]),
    "ssr_stoi": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _sz, _vp]),
    "ssr_stoi_band_edges": (_i, [_vp, _vp]),
    "ssr_wave_metrics_workspace_bytes": (_sz, [_vp, _i, _vp, _i, _i, _i]),
    "ssr_wave_metrics": (_i, [_vp, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "ssr_bss_sdr_workspace_bytes": (_sz, [_vp, _i, _vp, _i, _i]),
    "ssr_bss_sdr": (_i, [_vp, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "ssr_quality_metrics_workspace_bytes": (_sz, [_vp, _i, _vp, _i, _i, _i, _i]),
    "ssr_quality_metrics": (_i, [_vp, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "ssr_quality_bands": (_i, [_i, _vp, _vp, _vp, _vp, _sz]),
    "ssr_phase_metrics_workspace_bytes": (_sz, [_vp, _i, _vp, _i, _i, _i, _i]),
    "ssr_phase_metrics": (_i, [_vp, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "ssr_mrstft_workspace_bytes": (_sz, [_vp, _i, _vp, _i, _i, _vp, _vp, _vp]),
    "ssr_mrstft_metrics": (_i, [_vp, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, C.c_double, _vp, _vp, _sz,
                                _vp]),
    "ssr_f0_track_workspace_bytes": (_sz, [_vp, _i, C.c_double, C.c_double]),
    "ssr_f0_track": (_i, [_vp, _vp, _vp, _i, C.c_double, C.c_double, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "ssr_f0_metrics_workspace_bytes": (_sz, [_vp, _i, _vp, _i, C.c_double, C.c_double, _i]),
    "ssr_f0_metrics": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _i, C.c_double, C.c_double, _i, _vp, _vp, _sz, _vp]),
    "ssr_bootstrap_means": (_i, [_vp, _i64, _i, _vp, _i, _i, C.c_uint64, _i, _vp, _vp]),
    "ssr_bootstrap_summary": (_i, [_vp, _i, _i, _vp, _i, _vp, _vp, _vp]),
    "ssr_bootstrap_geometry": (_i, [C.POINTER(_i), C.POINTER(_i)]),
    "ssr_to_log": (_i, [_vp, _i64, _vp, _vp]),
    "ssr_from_log": (_i, [_vp, _i64, _vp, _vp]),
    "ssr_energy_sums": (_i, [_vp, _vp, _i, _i64, _vp, _vp]),
    "ssr_scale_items": (_i, [_vp, _vp, _vp, _i, _i64, _vp, _vp]),
    "ssr_sispec_multichannel": (_i, [_vp, _vp, _i, _i, _i64, _i, _vp, _vp, _sz, _vp]),
    "ssr_ola_workspace_bytes": (_sz, [_vp, _i64]),
    "ssr_fft_lowpass": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i64, _vp, _vp, _sz, _vp]),
    "ssr_fft_lowpass_multi": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _i, _i64, _vp, _i64, _vp, _sz, _vp]),
    "ssr_istft": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i64, _vp, _vp, _sz, _vp]),
    "ssr_resample_plan": (_i, [_i64, _i, _i, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i64), C.POINTER(_i),
                               C.POINTER(_i), C.POINTER(_i)]),
    "ssr_resample_poly": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _i, _i, _vp, _vp]),
    "ssr_resample_poly_chain": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _i, _i, _i, _i, _vp, _i, _i, _vp, _vp]),
    "ssr_resample_poly_mfma": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _i, _i, _vp, _vp]),
    "ssr_resample_poly_f64": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _i, _i, _vp, _vp]),
    "ssr_resample_sinc": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _i64, _vp, _vp, _i, _i, _i, C.c_double, C.c_double, _i,
                                _vp, _vp]),
    "ssr_pcm16_to_float": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp]),
    "ssr_flac_info": (_i, [C.c_char_p, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i64), C.POINTER(_i)]),
    "ssr_flac_decode_pcm16": (_i, [C.c_char_p, _vp, _i64, _i, C.POINTER(_i64)]),
    "ssr_flac_decode_i32": (_i, [C.c_char_p, _vp, _i64, _i, C.POINTER(_i64)]),
    "ssr_xcorr_workspace_bytes": (_sz, [_i, _i]),
    "ssr_xcorr_argmax": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _sz, _vp]),
    "ssr_sosfiltfilt_workspace_bytes": (_sz, [_i64, _i, _i]),
    "ssr_sosfiltfilt": (_i, [_vp, _vp, _vp, _i, _i64, _vp, _vp, _i, _i, _vp, _vp, _sz, _vp]),
    "ssr_sosfiltfilt_f64": (_i, [_vp, _vp, _vp, _i, _i64, _vp, _vp, _i, _i, _vp, _vp, _sz, _vp]),
    "ssr_sosfiltfilt_multi_workspace_bytes": (_sz, [_i64, _i, _vp, _i]),
    "ssr_sosfiltfilt_multi": (_i, [_vp, _vp, _vp, _i, _i64, _vp, _vp, _vp, _vp, _i, _vp, _i64, _vp, _sz, _vp]),
    "ssr_sosfiltfilt_fast_workspace_bytes": (_sz, [_i64, _i, _vp, _i]),
    "ssr_sosfiltfilt_fast": (_i, [_vp, _vp, _vp, _i, _i64, _vp, _vp, _vp, _vp, _i, _vp, _i64, _vp, _sz, _vp]),
    "ssr_sosfiltfilt_fast_f64": (_i, [_vp, _vp, _vp, _i, _i64, _vp, _vp, _vp, _vp, _i, _vp, _i64, _vp, _sz, _vp]),
    "ssr_comm_unique_id": (_i, [_vp]),
    "ssr_comm_init_rank": (_i, [_vp, _i, _i, C.POINTER(C.c_void_p)]),
    "ssr_comm_destroy": (_i, [_vp]),
    "ssr_allreduce_sums": (_i, [_vp, _i, _vp, _vp]),
}
# name -> (restype, argtypes): exactly the symbols ssr_eval_amd/csrc/ssr_hip_coherence.h declares (include/ssr_hip.h includes it)
COHERENCE_SIGNATURES = {
    "ssr_coherence_workspace_bytes": (_sz, [_vp, _i, _vp, _i, _i, _i, _i]),
    "ssr_coherence": (_i, [_vp, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _i, _vp, C.c_double, _vp, _vp, _vp, _sz, _vp]),
}
# name -> (restype, argtypes): exactly the symbols ssr_eval_amd/csrc/ssr_hip_loudness.h declares (include/ssr_hip.h includes it)
LOUDNESS_SIGNATURES = {
    "ssr_loudness_workspace_bytes": (_sz, [_vp, _i, _i]),
    "ssr_loudness": (_i, [_vp, _i, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
}
# name -> (restype, argtypes): exactly the symbols ssr_eval_amd/csrc/ssr_hip_spectrum.h declares (include/ssr_hip.h includes it)
SPECTRUM_SIGNATURES = {
    "ssr_spectrum_workspace_bytes": (_sz, [_vp, _i, _vp, _i, _i, _i, _i]),
    "ssr_spectrum": (_i, [_vp, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, C.c_double, C.c_double, _i, _vp, _vp, _vp, _vp, _vp,
                          _vp, _sz, _vp]),
}
# name -> (restype, argtypes): exactly the symbols ssr_eval_amd/csrc/ssr_hip_auditory.h declares (include/ssr_hip.h includes it)
AUDITORY_SIGNATURES = {
    "ssr_auditory_workspace_bytes": (_sz, [_vp, _i, _vp, _i, _i, _i]),
    "ssr_auditory": (_i, [_vp, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _vp, C.c_double, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
}
# name -> (restype, argtypes): exactly the symbols ssr_eval_amd/csrc/ssr_hip_modulation.h declares (include/ssr_hip.h includes it)
MODULATION_SIGNATURES = {
    "ssr_modulation_workspace_bytes": (_sz, [_vp, _i, _vp, _i, _i, _i]),
    "ssr_modulation": (_i, [_vp, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _i, _vp, C.c_double, _vp, _vp, _vp, _vp, _vp, _sz,
                            _vp]),
}
# name -> (restype, argtypes): exactly the symbols ssr_eval_amd/csrc/ssr_hip_distribution.h declares (include/ssr_hip.h includes it)
DISTRIBUTION_SIGNATURES = {
    "ssr_frechet_workspace_bytes": (_sz, [_vp, _i, _i]),
    "ssr_frechet": (_i, [_vp, _i, _vp, _vp, _i, _i, _i64, _i, _vp, _vp, _vp, _sz, _vp]),
    "ssr_kernel_distance_workspace_bytes": (_sz, [_vp, _i, _i, _i]),
    "ssr_kernel_distance": (_i, [_vp, _i, _vp, _vp, _i, _i, _i64, _vp, _i, C.c_double, _vp, _vp, _sz, _vp]),
    "ssr_pairwise_distances": (_i, [_vp, _i, _i64, _i64, _i, _i64, _vp, _i, _vp, _vp, _sz, _vp]),
}

# name -> (restype, argtypes): exactly the symbols ssr_eval_amd/csrc/ssr_hip_csii.h declares (include/ssr_hip.h includes it)
CSII_SIGNATURES = {
    "ssr_csii_workspace_bytes": (_sz, [_vp, _i, _vp, _i, _i, _i, _i]),
    "ssr_csii": (_i, [_vp, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
}
# name -> (restype, argtypes): exactly the symbols ssr_eval_amd/csrc/ssr_hip_align.h declares (include/ssr_hip.h includes it)
ALIGN_SIGNATURES = {
    "ssr_align_workspace_bytes": (_sz, [_vp, _i, _vp, _vp, _i, _i]),
    "ssr_align": (_i, [_vp, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
}
# name -> (restype, argtypes): exactly the symbols ssr_eval_amd/csrc/ssr_hip_nmr.h declares (include/ssr_hip.h includes it)
NMR_SIGNATURES = {
    "ssr_nmr_workspace_bytes": (_sz, [_vp, _i, _vp, _i, _i, _i]),
    "ssr_nmr": (_i, [_vp, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
}

_lib = None


class SsrHipError(RuntimeError):
    pass


def load():
    """Load libssrhip.so and bind every declared symbol; raises if the library was not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SsrHipError(
            "libssrhip.so not found at %s - build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  ssr_eval_amd has no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in list(SIGNATURES.items()) + list(COHERENCE_SIGNATURES.items()) + list(LOUDNESS_SIGNATURES.items()) + \
            list(SPECTRUM_SIGNATURES.items()) + list(AUDITORY_SIGNATURES.items()) + list(MODULATION_SIGNATURES.items()) + \
            list(DISTRIBUTION_SIGNATURES.items()) + list(CSII_SIGNATURES.items()) + list(ALIGN_SIGNATURES.items()) + list(NMR_SIGNATURES.items()):
        fn = getattr(lib, name)          # AttributeError here = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        msg = load().ssr_last_error()
        raise SsrHipError("libssrhip error %d: %s" % (rc, msg.decode() if msg else "?"))
