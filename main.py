"""Thin command line over vm_asr_amd with the reference's flags (main.py:28-318): train / --eval / --inference on the HIP path.

    python main.py --cfg configs/vm_asr_48k_MPD.yaml --synthetic 64                 # train (one process per GPU)
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 main.py --cfg ... --synthetic 512
    python main.py --cfg ... --eval --resume logs/.../ --tag 16000_48000 --synthetic 8 --degrade
    python main.py --cfg ... --inference --input speech.wav --resume logs/.../ --tag 16000_48000     # or --input <directory>
    python main.py --cfg ... --data-path data/                                      # train on <data>/<DST_PATH>/<speaker>/*.wav
    python main.py --cfg ... --data-path data/ --eval --resume logs/.../ --tag 16000_48000

`--cfg` takes the reference's yaml files unchanged.  The VCTK pipeline (download, flac decoding, dataset splits:
data_loader/data_loaders.py) is out of scope: clips come from `--synthetic N` (trainer.SyntheticVCTK, the
reference's batch contract) — a real dataset plugs in as any DataLoader yielding `(wave_in, wave_tgt, highcut, name,
pad)`.  `--data-path DIR` sets DATA.DATA_PATH and takes the clips from the wav files below it instead (vm_asr_amd.data: the
reference's speaker split, validation split and test loader; resampling, noise tail and the input degradation run on the
device); it excludes `--synthetic`.  `--degrade` replaces each clip's input by the reference's degradation of its target, computed on the device
(vm_asr_amd.resample.DegradeOnDevice: resampled down and up again; the rate is TAG's under --eval, a seeded draw from
DATA.RANDOM_RESAMPLE per clip in training).  `--inference --input <wav file or directory>` enhances wav files
(vm_asr_amd.inferencer) and writes `{stem}_enhanced.wav`; `--throughput` runs bench.py's measurement.
"""
import argparse
import os

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")   # vm_asr_amd/hip_env.py: before the GPU is initialised
os.environ.setdefault("TENSILE_STREAMK_DATA_PARALLEL", "1")   # vm_asr_amd/hip_env.py: stream-K GEMMs of two streams can stall the device
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def parse_option(argv=None):
    p = argparse.ArgumentParser("VM-ASR (MI355X) training and evaluation")
    p.add_argument("--cfg", type=str, required=True, metavar="FILE")
    p.add_argument("--opts", default=None, nargs="+", help="KEY VALUE pairs")
    p.add_argument("--batch-size", type=int)
    p.add_argument("--input_sr", type=int)
    p.add_argument("--target_sr", type=int)
    p.add_argument("--resume", type=str)
    p.add_argument("--accumulation-steps", type=int)
    p.add_argument("--disable_amp", action="store_true")
    p.add_argument("--output", default="logs", type=str)
    p.add_argument("--tag", default=time.strftime("%Y%m%d%H%M%S", time.localtime()))
    p.add_argument("--eval", action="store_true")
    p.add_argument("--inference", action="store_true")
    p.add_argument("--input", type=str)
    p.add_argument("--throughput", action="store_true")
    p.add_argument("--synthetic", type=int, default=None, help="number of synthetic VCTK-shaped clips per epoch (default 64)")
    p.add_argument("--data-path", type=str, metavar="DIR",
                   help="train / evaluate on the wav files of DIR/<DATA.FLAC2WAV.DST_PATH>/<speaker>/ (vm_asr_amd.data) instead of synthetic clips")
    p.add_argument("--epochs", type=int, help="override TRAIN.EPOCHS")
    p.add_argument("--no-graphs", action="store_true", help="run the step eagerly instead of replaying HIP graphs")
    p.add_argument("--degrade", action="store_true",
                   help="make each clip's input from its target on the device: resampled down and up again (resample.DegradeOnDevice)")
    p.add_argument("--segment-batch", type=int, default=1, help="--inference: segments of a long file per generator call")
    p.add_argument("--step-metrics", action="store_true",
                   help="metrics on every step / clip through the fused kernel (Trainer step_metrics, Tester fused_metrics)")
    p.add_argument("--skip-nonfinite", action="store_true",
                   help="do not take an optimiser step whose gradients hold an inf or a NaN (device-side gradient guard, one per optimiser)")
    p.add_argument("--clip-grad", type=float, default=None, metavar="FLOAT",
                   help="clip each optimiser's gradients to this global L2 norm on the device (implies the guard of --skip-nonfinite)")
    args = p.parse_args(argv)
    if args.data_path and args.synthetic is not None:
        p.error("--data-path and --synthetic exclude each other")
    if args.synthetic is None:
        args.synthetic = 64
    from vm_asr_amd.config import get_config
    opts = list(args.opts or [])
    if args.data_path:
        opts += ["DATA.DATA_PATH", args.data_path]
    if args.target_sr:
        opts += ["DATA.TARGET_SR", args.target_sr]
    if args.epochs:
        opts += ["TRAIN.EPOCHS", args.epochs]
    config = get_config(args.cfg, opts, batch_size=args.batch_size, resume=args.resume, accumulation_steps=args.accumulation_steps,
                        disable_amp=args.disable_amp, output=args.output, tag=args.tag, eval=args.eval, inference=args.inference,
                        throughput=args.throughput, input_sr=args.input_sr)
    return args, config


def use_graphs(args, config):
    """Whether training replays HIP graphs: the default, except under --no-graphs, with gradient accumulation, and when the multi-scale
    discriminator is listed (its step is eager only: Trainer.enable_graphs raises; the optimisers are then built non-capturable too)."""
    adv = config.TRAIN.ADVERSARIAL
    return not args.no_graphs and config.TRAIN.ACCUMULATION_STEPS == 1 and not (adv.ENABLE and "msd" in adv.DISCRIMINATORS)


def main(args, config):
    import vm_asr_amd
    from vm_asr_amd.trainer import (SyntheticVCTK, Trainer, _Logger, build_optimizer, build_scheduler, default_metric_ftns,
                                    init_distributed)
    log = _Logger()
    if config.INFERENCE_MODE and not args.input:
        raise SystemExit("--inference needs --input <wav file or directory>")
    if config.THROUGHPUT_MODE:
        import subprocess
        raise SystemExit(subprocess.call([sys.executable, os.path.join(ROOT, "bench.py")]))   # child process, exit with its code
    rank, local, world = init_distributed()
    if not torch.cuda.is_available():
        raise SystemExit("vm_asr_amd needs a GPU (there is no CPU path)")
    device = torch.device("cuda", local % torch.cuda.device_count())
    torch.cuda.set_device(device)
    torch.manual_seed(config.SEED)
    models = vm_asr_amd.get_model(config)
    if config.INFERENCE_MODE:
        from vm_asr_amd.inferencer import Inferencer
        inf = Inferencer({"generator": models["generator"]}, config, device, log, segment_batch=args.segment_batch)
        if os.path.isdir(args.input):
            print("\n".join(inf.infer_directory(args.input)))
        else:
            inf.infer_file(args.input)
        return
    metrics = default_metric_ftns(config)
    sr_in = args.input_sr or (16000 if config.DATA.TARGET_SR == 48000 else 8000)
    if config.EVAL_MODE:
        from vm_asr_amd.tester import Tester
        if args.data_path:
            from vm_asr_amd.data import get_loader
            loader = get_loader(config, device, log)
        else:
            ds = SyntheticVCTK(config, length=args.synthetic, sr_in=sr_in, seed=config.SEED + 10_000)
            loader = torch.utils.data.DataLoader(ds, batch_size=1, shuffle=False)
        if args.degrade and not args.data_path:
            from vm_asr_amd.resample import DegradeOnDevice
            loader = DegradeOnDevice(loader, config, device, sr_input=int(str(config.TAG).split("_")[0]))
        res = Tester({"generator": models["generator"]}, metrics, config, device, loader, log, fused_metrics=args.step_metrics).evaluate()
        print({k: round(v, 4) if isinstance(v, float) else v for k, v in res.items()})
        return
    gan = config.TRAIN.ADVERSARIAL.ENABLE
    graphs = use_graphs(args, config)
    val_loader = None
    if args.data_path:
        from vm_asr_amd.data import get_loader
        loader, val_loader = get_loader(config, device, log, drop_last=graphs)
    else:
        ds = SyntheticVCTK(config, length=args.synthetic, sr_in=sr_in, seed=config.SEED + 1000 * rank)
        loader = torch.utils.data.DataLoader(ds, batch_size=config.DATA.BATCH_SIZE, shuffle=False, drop_last=True)
        if args.degrade:
            from vm_asr_amd.resample import DegradeOnDevice
            loader = DegradeOnDevice(loader, config, device, seed=config.SEED + 1000 * rank)
    for m in models.values():
        if m is not None:
            m.to(device)
    opts = {"generator": build_optimizer(config, models["generator"], capturable=graphs)}
    if gan:
        opts["discriminator"] = build_optimizer(config, [models[d] for d in config.TRAIN.ADVERSARIAL.DISCRIMINATORS], capturable=graphs)
    steps = max(1, len(loader) // config.TRAIN.ACCUMULATION_STEPS)
    sched = {k: build_scheduler(config, o, steps) for k, o in opts.items()}      # TRAIN.LR_SCHEDULER.NAME: cosine | linear | step | multistep
    tr = Trainer(models, metrics, opts, config, device, loader, val_loader, sched, amp=config.AMP_ENABLE, gan=gan, logger=log,
                 step_metrics=args.step_metrics, skip_nonfinite=args.skip_nonfinite, clip_grad=args.clip_grad)
    if gan and "msd" in config.TRAIN.ADVERSARIAL.DISCRIMINATORS and not args.no_graphs:
        log.info("DISCRIMINATORS lists 'msd': the step runs eagerly (no HIP graphs), as under --no-graphs")
    if graphs:
        first = next(iter(loader))
        tr.enable_graphs(tr._to_dev(first))
    tr.train()


if __name__ == "__main__":
    main(*parse_option())
