#!/usr/bin/env python3
"""Sliding-window laughter segmentation of one audio file on the MI355X.

Counterpart of the reference's segment_laughter.py (argparse :28-40, model load :59-74, `load_and_pred` :79-122,
`save_instances` :124-161): same flags, same outputs (one TextGrid per (threshold, min_length) setting under
`<output_dir>/t_<thr>/l_<min_len>/`).  What changes is the loop: the reference moves 32 windows at a time through the
model (11,250 host round trips for a 60 min channel); here the whole file is featurised in one launch and
`engine.predict_windows` reads the stride-one-frame windows straight from the (T, 44) matrix, in chunks of
`engine.PREDICT_CHUNK[precision]` windows (the sizes bench.py measures).  `--precision fp32` (default) is the reference's
arithmetic; `--precision fp16` runs the convolutions on the 16-bit matrix cores (BASELINE configs[4]: about 30x faster;
tolerance in tests/test_resnet_gpu.py) -- the invocation behind the published real-time factor is

    python segment_laughter.py --config resnet_base --model_path <dir> --input_audio_file <wav> --output_dir <out> \\
        --precision fp16 --thresholds 0.1,...  --min_lengths 0.0,0.1,0.2

The script prints the real-time factor of everything it does (file read, featurisation, windows, threshold sweep,
TextGrid / wav output).  With torchrun (one process per GPU) the window range is sharded over ranks and the
probabilities are all-gathered.

`--segmenter device` (default `host`) keeps the gathered track on the GPU and cuts it there (csrc/runs.hip through
`laugh_segmenter.get_laughter_instances_device`: the run tables of every threshold in four launches); only the compact tables
cross to the host, and the track itself only when `--save_probs` asks for it.  Same TextGrids and wav files, byte for byte.

`--lowpass CUTOFF` (default: off) smooths the track before the sweep with the reference's `lowpass` (laugh_segmenter.py:49-55,
which segment_laughter.py:107-108 leaves commented out): scipy on the host under `--segmenter host`, csrc/lowpass.hip under
`--segmenter device`, where the track still never leaves the GPU.  `--save_probs` keeps writing the raw track.

`--median FRAMES` (default: off; not in the reference) passes the track through a median filter of FRAMES frames before the sweep
(odd, 1..1023, the ends replicated): laugh_segmenter.median_filter under `--segmenter host`, csrc/rankfilt.hip under `--segmenter
device` -- the same values bit for bit, so the same files.  Not together with `--lowpass`; `--save_probs` keeps writing the raw track.

`--offset_drops` / `--min_gaps` (default: absent) add hysteresis and gap filling (laugh_segmenter.binarize_instances, or
csrc/binarize.hip under `--segmenter device`): the instances of setting (thr, drop, gap, min_len) go to
`t_<thr>/l_<min_len>/d_<drop>_g_<gap>/`.  Without the two flags paths and bytes are what they were.

`--penalties` (default: absent) cuts the track with the two-state Viterbi decoder instead (laugh_segmenter.viterbi_instances, or
csrc/viterbi.hip under `--segmenter device`): log-odds relative to the threshold, a penalty in nats per instance.  The instances of
setting (thr, penalty, min_len) go to `t_<thr>/l_<min_len>/p_<penalty>/`.  It cannot be combined with the two flags above.

`--confidence True` (default: off; not in the reference) writes `<file>.confidence.csv` next to every TextGrid: one line per
instance, `start,end,mean_prob,peak_time,peak_prob` (laugh_segmenter.span_stats / confidences, or csrc/spanstats.hip under
`--segmenter device`: the same integers, so the same bytes).  `--min_confidence X` drops the instances whose mean probability is
below X before anything is printed, cut or written.  Both work with either segmenter and every decoder; with `--lowpass` or
`--median` the figures are those of the smoothed track, the one the instances were cut from.  Without the two flags paths and bytes
are what they were; the TextGrid format never changes.

`--calibration FILE` (default: absent; not in the reference) applies the table of a `calibration_table.npz` that
`evaluate_sweep.py --fit_calibration` wrote to the track first, before `--lowpass` / `--median` and every decoder
(laugh_segmenter.apply_calibration under `--segmenter host`, csrc/calibration.hip under `--segmenter device`: the same values bit
for bit).  Thresholds, penalties in nats and `--confidence` then speak of calibrated probabilities; `--save_probs` keeps writing
the raw track.
"""
import argparse
import os
import sys
import time

_PKG = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.join(_PKG, "utils"), _PKG):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import audio_utils  # noqa: E402
import config as config_mod  # noqa: E402
from evaluate_sweep import cutoff_arg, float_list, window_arg  # noqa: E402  (the argparse types of --lowpass, --median and the decoders' lists)
import laugh_segmenter  # noqa: E402
import load_data  # noqa: E402
import parallel  # noqa: E402
import textgrid  # noqa: E402
import torch_utils  # noqa: E402


def build_model(config_name, model_path, device):
    config = config_mod.MODEL_MAP[config_name]
    model = config['model'](dropout_rate=0.0, linear_layer_size=config['linear_layer_size'],
                            filter_sizes=config['filter_sizes'])
    model.set_device(device)
    ckpt = os.path.join(model_path, 'best.pth.tar')
    if os.path.exists(ckpt):
        torch_utils.load_checkpoint(ckpt, model, map_location=device)
        model.eval()
    else:
        raise Exception(f"Model checkpoint not found at {model_path}")
    return model


def predict_file_device(model, audio_path, chunk=None, rank=0, world=1, precision="fp32", resample=False):
    """probs (T,) float32 GPU tensor for the stride-one-frame windows of the file + its duration in seconds.
    chunk=None: the engine's own chunk size for the precision (engine.PREDICT_CHUNK).  resample=True: a file at another rate than
    16 kHz is converted on the GPU (csrc/resample.hip) instead of refused; its duration stays frames over its own rate."""
    loader = load_data.create_inference_dataloader(audio_path, resample=resample)
    feats = loader.dataset.feats
    T = feats.shape[0]
    sh = parallel.shard_indices(T, rank, world)
    local = model.engine.predict_windows(feats, n_frames=loader.dataset.n_frames, chunk=chunk, start=sh.start, stop=sh.stop,
                                         precision=precision)
    probs = parallel.gather_probs(local, T, rank, world)
    file_length = audio_utils.get_audio_length(audio_path)  # seconds; fps = T / file_length (segment_laughter.py:103-104)
    return probs, file_length


def predict_file(model, audio_path, chunk=None, rank=0, world=1, precision="fp32", resample=False):
    """predict_file_device with the track copied to the host: probs (T,) float32 numpy + the duration in seconds."""
    probs, file_length = predict_file_device(model, audio_path, chunk=chunk, rank=rank, world=world, precision=precision,
                                             resample=resample)
    return probs.cpu().numpy(), file_length


def save_audio_instances(instances, audio_path, output_dir, rate=None):
    """One `laugh_<i>.wav` per instance (segment_laughter.py:133-149).  The reference re-reads the file with
    `librosa.load(sr=44100)`, i.e. resampled.  rate=None: the cut is taken from the file's own samples at its own rate;
    rate=44100 (or any other): the file is converted once on the GPU to that rate (load_data.load_audio_device) and the
    instances are cut from that -- the reference's behaviour.  Same instants, same int16 scaling (`maxv = 32767`)."""
    from scipy.io import wavfile
    sr = audio_utils.get_sampling_rate(audio_path)
    if rate is None or int(rate) == sr:
        y = load_data.load_audio(audio_path, sampling_rate=sr)
    else:
        y = load_data.load_audio_device(audio_path, sampling_rate=int(rate), device=torch.device('cuda', torch.cuda.current_device()),
                                        resample=True, source_rate=sr).cpu().numpy()
        sr = int(rate)
    maxv = np.iinfo(np.int16).max
    paths = []
    for index, instance in enumerate(instances):
        laughs = laugh_segmenter.cut_laughter_segments([instance], y, sr)
        wav_path = os.path.join(output_dir, "laugh_" + str(index) + ".wav")
        wavfile.write(wav_path, sr, (np.asarray(laughs, dtype=np.float64) * maxv).astype(np.int16))
        paths.append(wav_path)
    return paths


def write_confidence_csv(path, instances, conf):
    """start,end,mean_prob,peak_time,peak_prob: one line per instance, floats as repr (conf: the (n, 3) array of the instances)."""
    with open(path, "w") as f:
        f.write("start,end,mean_prob,peak_time,peak_prob\n")
        for (start, end), row in zip(instances, conf.tolist()):
            f.write(",".join(repr(float(v)) for v in (start, end, *row)) + "\n")


def load_and_pred(model, audio_path, thresholds, min_lengths, output_dir, save_to_textgrid=True, rank=0, world=1,
                  precision="fp32", save_to_audio_files=False, verbose=True, save_probs=None, segmenter="host", resample=False,
                  save_audio_rate=None, lowpass=None, offset_drops=None, min_gaps=None, penalties=None, median=None, confidence=False,
                  min_confidence=None):
    """segment_laughter.py:79-122: load_and_pred_calibrated without a calibration table (its docstring has the arguments)."""
    return load_and_pred_calibrated(model, audio_path, thresholds, min_lengths, output_dir, save_to_textgrid, rank, world, precision,
                                    save_to_audio_files, verbose, save_probs, segmenter, resample, save_audio_rate, lowpass, offset_drops,
                                    min_gaps, penalties, median, confidence, min_confidence)


def load_and_pred_calibrated(model, audio_path, thresholds, min_lengths, output_dir, save_to_textgrid=True, rank=0, world=1,
                             precision="fp32", save_to_audio_files=False, verbose=True, save_probs=None, segmenter="host", resample=False,
                             save_audio_rate=None, lowpass=None, offset_drops=None, min_gaps=None, penalties=None, median=None,
                             confidence=False, min_confidence=None, *, calibration=None):
    """segment_laughter.py:79-122.  Returns (seconds taken by everything below, {(thr, min_len): [(start, end), ...]}).
    segmenter "device": the track stays on the GPU and rank 0 cuts it there (the other ranks return an empty dictionary).
    resample: accept a file at another rate than 16 kHz (converted on the GPU).  save_audio_rate: rate of the laugh_<i>.wav cuts
    (None: the file's own).  lowpass: a cutoff (of Nyquist): the track is smoothed before the sweep (segment_laughter.py:107-108), on
    the host or on the device like the sweep itself; save_probs still gets the raw track.  median: a window in frames (odd,
    1..1023): the track goes through the median filter instead (laugh_segmenter.median_filter / median_filter_device); not both.
    offset_drops / min_gaps (either given): hysteresis and gap filling; the dictionary's keys are (thr, drop, gap, min_len).
    penalties: the Viterbi decoder; the dictionary's keys are (thr, penalty, min_len).  Not together with the two above.
    confidence: also write <file>.confidence.csv next to every TextGrid (start,end,mean_prob,peak_time,peak_prob per instance, of
    the track the instances were cut from: the smoothed one under lowpass / median).  min_confidence: instances whose mean
    probability lies below it are dropped from the dictionary and from everything printed, cut or written.
    calibration: None, or a calibration table (float64 (65537,): calibration.load_table): applied to the track first, in front of the
    smoother and the decoder, on the host or on the device like the sweep; save_probs still gets the raw track."""
    if segmenter not in ("host", "device"):
        raise ValueError(f"segmenter must be 'host' or 'device', got {segmenter!r}")
    if lowpass is not None and median is not None:
        raise ValueError("lowpass and median are two smoothers for the same place: give one of them")
    if save_to_audio_files and output_dir is None:
        raise Exception("Need to specify an output directory to save audio files")   # segment_laughter.py:138-140
    start_time = time.time()
    predict = predict_file_device if segmenter == "device" else predict_file
    probs, file_length = predict(model, audio_path, rank=rank, world=world, precision=precision, resample=resample)
    if segmenter == "device":
        torch.cuda.synchronize(probs.device)   # (the host path's copy waits for the model pass: the same split of the two legs)
    predict_time = time.time() - start_time
    if save_probs and rank == 0:
        # (not in the reference: the per-frame track, e.g. to compare a sharded run with a single-rank one)
        np.save(save_probs, probs.cpu().numpy() if segmenter == "device" else probs)
    fps = len(probs) / float(file_length)
    if calibration is not None and (segmenter == "host" or rank == 0):
        probs = laugh_segmenter.apply_calibration(probs, calibration) if segmenter == "host" else \
            laugh_segmenter.apply_calibration_device(probs, calibration)
    if lowpass is not None and (segmenter == "host" or rank == 0):
        probs = laugh_segmenter.lowpass(probs, cutoff=lowpass) if segmenter == "host" else \
            laugh_segmenter.lowpass_device(probs, cutoff=lowpass)
    elif median is not None and (segmenter == "host" or rank == 0):
        probs = laugh_segmenter.median_filter(probs, median) if segmenter == "host" else \
            laugh_segmenter.median_filter_device(probs, median)
    decoder, axis_values = laugh_segmenter.decoder_for(offset_drops, min_gaps, penalties)
    want_stats = bool(confidence) or min_confidence is not None
    stats_dict = {}
    if segmenter == "host" or rank == 0:
        instance_dict = laugh_segmenter._instances(decoder, probs, thresholds, min_lengths, fps, axis_values, device=segmenter == "device",
                                                   stats=want_stats)
        if want_stats:
            instance_dict, stats_dict = instance_dict
        if min_confidence is not None:
            for setting, conf in stats_dict.items():
                keep = ~(conf[:, 0] < min_confidence)
                instance_dict[setting] = [inst for inst, k in zip(instance_dict[setting], keep) if k]
                stats_dict[setting] = conf[keep]
    else:
        instance_dict = {}
    sweep_time = time.time() - start_time - predict_time
    if rank == 0:
        for setting, instances in instance_dict.items():
            if verbose:
                print(decoder.found_line(len(instances), setting))
            out_dir = os.path.join(output_dir or '.', f't_{setting[0]}', f'l_{setting[-1]}', *decoder.dir_suffix(setting))
            if save_to_textgrid or confidence or (save_to_audio_files and len(instances) > 0):
                os.makedirs(out_dir, exist_ok=True)
            if save_to_audio_files and len(instances) > 0:
                wav_paths = save_audio_instances(instances, audio_path, out_dir, rate=save_audio_rate)
                if verbose:
                    print(laugh_segmenter.format_outputs(instances, wav_paths))   # segment_laughter.py:148
            fname = os.path.splitext(os.path.basename(audio_path))[0]
            if save_to_textgrid:
                textgrid.write_laughter_textgrid(os.path.join(out_dir, fname + '.TextGrid'), instances, xmax=file_length)
            if confidence:
                write_confidence_csv(os.path.join(out_dir, fname + '.confidence.csv'), instances, stats_dict[setting])
    time_taken = time.time() - start_time
    if rank == 0:
        print(f'Completed in: {time_taken:.2f}s  (real-time factor of the whole script {time_taken / file_length:.2e} at '
              f'{precision}: read + featurise + {len(probs)} windows {predict_time:.3f}s, '
              f'{len(instance_dict)}-setting sweep {sweep_time:.3f}s, output {time_taken - predict_time - sweep_time:.3f}s)')
    return time_taken, instance_dict


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument('--model_path', type=str, default='checkpoints/in_use/resnet_with_augmentation')
    parser.add_argument('--config', type=str, default='resnet_base')
    parser.add_argument('--thresholds', type=str, default='0.5', help='Single value or comma-separated list of thresholds to evaluate')
    parser.add_argument('--min_lengths', type=str, default='0.2', help='Single value or comma-separated list of min_lengths to evaluate')
    parser.add_argument('--input_audio_file', required=True, type=str)
    parser.add_argument('--output_dir', type=str, default=None)
    parser.add_argument('--save_to_audio_files', type=str, default='False',
                        help="laugh_<i>.wav per instance, cut from the file at its own sampling rate or at --save_audio_rate (the reference "
                             "resamples to 44.1 kHz with librosa and defaults this flag to 'True'; here it is opt-in: it needs --output_dir)")
    parser.add_argument('--save_probs', type=str, default=None, help='(not in the reference) write the per-frame probabilities to this .npy')
    parser.add_argument('--save_to_textgrid', type=str, default='True')
    parser.add_argument('--gpus', type=int, default=None,
                        help='ranks that share the window range; > 1 without a launcher environment starts the ranks itself')
    parser.add_argument('--precision', type=str, default='fp32', choices=['fp32', 'fp16'], help='matrix-core precision')
    parser.add_argument('--segmenter', type=str, default='host', choices=['host', 'device'],
                        help="(not in the reference) where the probability track is cut into instances: 'host' copies it to the host "
                             "(numpy, one pass per threshold); 'device' cuts it on the GPU, all thresholds in one pass -- same output")
    parser.add_argument('--lowpass', type=cutoff_arg, default=None, metavar='CUTOFF',
                        help="smooth the probability track before the sweep: second-order Butterworth at CUTOFF of Nyquist, forwards "
                             "and backwards (the reference's lowpass, cutoff 0.01, which it leaves commented out); on the host or the "
                             "GPU as --segmenter says; default: off")
    parser.add_argument('--median', type=window_arg, default=None, metavar='FRAMES',
                        help="(not in the reference) pass the probability track through a median filter of FRAMES frames before the "
                             "sweep (odd, 1..1023, the ends replicated); on the host or the GPU as --segmenter says; not with --lowpass; "
                             "default: off")
    parser.add_argument('--offset_drops', type=float_list, default=None,
                        help="(not in the reference) comma-separated list: hysteresis, an instance that starts above a threshold lasts "
                             "until the track falls to or below threshold - drop; default: absent")
    parser.add_argument('--min_gaps', type=float_list, default=None,
                        help="(not in the reference) comma-separated list of seconds: instances separated by a pause of at most this "
                             "become one, before the min_length filter; default: absent")
    parser.add_argument('--penalties', type=float_list, default=None,
                        help="(not in the reference) comma-separated list of nats: two-state Viterbi decoding of the track, a frame "
                             "counting its log-odds relative to the threshold and every instance costing this much; default: absent")
    parser.add_argument('--confidence', type=str, default='False',
                        help="(not in the reference) 'True': write <file>.confidence.csv next to every TextGrid, one line per instance: "
                             "start,end,mean_prob,peak_time,peak_prob; with --lowpass or --median the figures are those of the smoothed "
                             "track, the one the instances were cut from; default: off")
    parser.add_argument('--min_confidence', type=float, default=None, metavar='X',
                        help="(not in the reference) drop the instances whose mean probability is below X before anything is printed, cut "
                             "or written (of the smoothed track under --lowpass or --median); default: absent")
    parser.add_argument('--calibration', type=str, default=None, metavar='FILE',
                        help="(not in the reference) a calibration_table.npz of evaluate_sweep.py --fit_calibration: its table is "
                             "applied to the track first, before --lowpass / --median and every decoder; default: absent")
    parser.add_argument('--resample', type=str, default='False',
                        help="(not in the reference) 'True': an input file at another sampling rate than 16 kHz is converted on the GPU "
                             "(polyphase FIR, scipy.signal.resample_poly's convention) instead of refused")
    parser.add_argument('--save_audio_rate', type=int, default=None,
                        help="sampling rate of the laugh_<i>.wav cuts: the file is converted to it once on the GPU (the reference writes "
                             "44100); default: the file's own rate, no conversion")
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.median is not None and args.lowpass is not None:
        raise SystemExit("--median cannot be combined with --lowpass: they are two smoothers for the same place")
    if args.gpus is not None and args.gpus > 1 and not parallel.under_launcher():
        raise SystemExit(parallel.spawn_ranks(args.gpus, os.path.abspath(__file__), sys.argv[1:] if argv is None else list(argv),
                                              timeout=None))
    thresholds = [float(t) for t in args.thresholds.split(',')]
    min_lengths = [float(l) for l in args.min_lengths.split(',')]
    table = None
    if args.calibration is not None:
        import calibration
        table = calibration.load_table(args.calibration)
    rank, world, local = parallel.init_from_env()
    if args.gpus is not None and world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but the launcher environment says WORLD_SIZE={world}")
    if not torch.cuda.is_available():
        raise SystemExit("segment_laughter.py needs an MI355X (the HIP path has no CPU fallback)")
    device = torch.device('cuda', local)
    torch.cuda.set_device(device)
    model = build_model(args.config, args.model_path, device)
    truthy = ('true', '1', 'yes')
    load_and_pred_calibrated(model, args.input_audio_file, thresholds, min_lengths, args.output_dir,
                             save_to_textgrid=args.save_to_textgrid.lower() in truthy, rank=rank, world=world, precision=args.precision,
                             save_to_audio_files=args.save_to_audio_files.lower() in truthy, save_probs=args.save_probs,
                             segmenter=args.segmenter, resample=args.resample.lower() in truthy, save_audio_rate=args.save_audio_rate,
                             lowpass=args.lowpass, offset_drops=args.offset_drops, min_gaps=args.min_gaps, penalties=args.penalties,
                             median=args.median, confidence=args.confidence.lower() in truthy, min_confidence=args.min_confidence,
                             calibration=table)


if __name__ == '__main__':
    main()
