"""Drop-in for the reference's config.py (config.py:7-31): same names, same keys, MI355X model class.

`ANALYSIS` (config.py:34-63) configures the transcript-evaluation tooling, which is outside the hot path
 and is not reproduced.
"""
import os
import sys

_PKG = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.join(_PKG, "utils"), _PKG):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import models  # noqa: E402

MODEL_MAP = {}

MODEL_MAP['resnet_base'] = {
    'batch_size': 32,
    'model': models.ResNetBigger,
    'val_data_text_path': './data/switchboard/val/switchboard_val_data.txt',
    'log_frequency': 900,
    'linear_layer_size': 48,  # features of shape (100, 44): 16 channels x 3 x 1 after AvgPool2d(4)
    'filter_sizes': [64, 32, 16, 16],
}

# The reference's default for segment_laughter.py.  It runs on the reference's original features, FEAT['num_samples'] = 128
# (128 x 44 windows: block4 leaves 32 channels x 16 x 6, AvgPool2d(4) -> 32 x 4 x 1 = 128 = linear_layer_size; config.py:14-15 of
# the reference).  On (100, 44) features it fails exactly as the reference does (flattened size 96 != 128 -> RuntimeError,
# SURVEY.md section 0).  These widths run on the exact-f32 kernels only (engine.ResNetEngine.base_widths): no split-operand or
# fp16 paths.
MODEL_MAP['resnet_with_augmentation'] = {
    'batch_size': 32,
    'model': models.ResNetBigger,
    'val_data_text_path': './data/switchboard/val/switchboard_val_data.txt',
    'log_frequency': 200,
    'linear_layer_size': 128,
    'filter_sizes': [128, 64, 32, 32],
}

FEAT = {
    "num_samples": 100,
    "num_filters": 44
}

# Train-time augmentation presets (augment.AugmentConfig fields; the convention is in include/lad_hip.h next to
# lad_gather_segments_aug).  The reference has none -- its 'resnet_with_augmentation' names a model, not a data path; the values are
# SpecAugment's usual ones scaled to one-second segments of 100 frames x 44 filters.
AUGMENT = {}

AUGMENT['spec'] = {
    'p': 0.9,
    'W': 5,                     # time warp: the centre frame moves by at most 4 frames
    'n_time': 2, 'Wt': 20,      # two frame masks of 0..20 frames
    'n_freq': 2, 'Wf': 8,       # two feature masks of 0..8 filters
}

AUGMENT['mix'] = {
    'mix_p': 0.5,
    'snr_lo': 5.0, 'snr_hi': 20.0,     # dB
    'gain_lo': -6.0, 'gain_hi': 6.0,   # dB
}

AUGMENT['spec+mix'] = {**AUGMENT['spec'], **AUGMENT['mix']}

# Segment-table presets (sampling.SegmentPools.plan; the convention is in include/lad_hip.h next to lad_sample_segments).
# 'reference' is create_data_df.py's scheme: per laugh row num_laugh_samples windows of the row and num_non_laugh_samples
# negatives, floor(0.7 n) of them silence, floor(0.1 n) noise, the rest speech (:124-126); random=True draws every negative from
# anywhere outside laughter and invalid regions (:144-147).  The reference reads the two counts from its environment
# (NUM_OF_LAUGH_SAMPLES / NUM_OF_NON_LAUGH_SAMPLES, :212-213) and ships no values: the ones here are this project's default.
SAMPLING = {}

SAMPLING['reference'] = {
    'num_laugh_samples': 10,
    'num_non_laugh_samples': 10,
    'silence_share': 0.7,
    'noise_share': 0.1,
    'subsample_duration': 1.0,  # seconds: the segment length (config.py:56 of the reference)
    'random': False,
}

# Hysteresis / gap-filling presets (keyword arguments of laugh_segmenter.binarize_instances and of the offset_drops= / min_gaps=
# axes of sweep_eval; the convention is in include/lad_hip.h next to lad_binarize_count).  The reference has neither control; 'off'
# is its rule (one threshold, no joining), 'sweep' the two extra axes tools/bench_binarize.py times.  Nothing reads this unless asked.
BINARIZE = {}

BINARIZE['off'] = {'offset_drops': [0.0], 'min_gaps': [0.0]}

BINARIZE['sweep'] = {'offset_drops': [0.0, 0.1, 0.2], 'min_gaps': [0.0, 0.1, 0.3]}
