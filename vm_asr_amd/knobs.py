"""Every VMASR_* environment switch, declared once: name, kind, default, allowed values, who reads it, what it does.

`get(name)` reads the environment AT CALL TIME (tests and tools change it between calls) and returns the parsed value; a value
outside the declared set raises ValueError at the read.  Nothing else under vm_asr_amd/ reads a VMASR_* variable.  Readers:
"python" = this package through get(), for the switches that existed when this registry was written: tests/test_knobs.py pins exactly
that set and its defaults in a fixed table.  A python-read switch added later cannot join the table, so it carries "python:<feature>"
(so far "python:msd", "python:gmlp", "python:sgd") and the tests of its feature check its default, its values and the ValueError of a bad one (tests/test_msd.py, tests/test_msd_stem.py, tests/test_msd_tail.py, tests/test_gmlp.py, tests/test_lr_schedules.py);
"csrc" = a static `getenv` in vm_asr_amd/csrc (read once per process; listed here with the
default the C++ code applies); "external" = bench.py, the tests, tools/ or oracle/, which read their own names directly.
No torch import: tests/test_knobs.py and tools load this module without a GPU stack.
"""
import os
import warnings
from collections import namedtuple

Knob = namedtuple("Knob", "name kind default values reader doc parse")


def _bad(k, raw, allowed):
    return ValueError(f"{k.name}={raw!r}: expected {allowed}")


def _flag(k, raw):
    if raw == "1":
        return True
    if raw == "0":
        return False
    raise _bad(k, raw, "0 or 1")


def _choice(k, raw):
    if raw in k.values:
        return raw
    raise _bad(k, raw, "one of " + " | ".join(k.values))


def _int(k, raw):
    try:
        return int(raw)
    except ValueError:
        raise _bad(k, raw, "an integer") from None


def _float(k, raw):
    try:
        return float(raw)
    except ValueError:
        raise _bad(k, raw, "a number") from None


def _str(k, raw):
    return raw or k.default          # (set but empty = unset, as `os.environ.get(name) or default` read it)


def _comma_list(k, raw):
    return tuple(raw.split(","))


def _step_variant(k, raw):
    """-> None (unset / empty) or the pinned layout (phase lane?, share of the CUs for the discriminator's backward or None)."""
    if raw == "":
        return None
    if raw == "one":
        return (False, None)
    if raw == "lane":
        return (True, None)
    if raw.startswith("lane:"):
        try:
            share = float(raw[5:])
        except ValueError:
            share = 0.0
        if 0.0 < share < 1.0:
            return (True, share)
    raise _bad(k, raw, "one | lane | lane:<share> with 0 < share < 1")


_PARSE = {"flag": _flag, "choice": _choice, "int": _int, "float": _float, "str": _str}
_FLAG_VALUES = ("0", "1")


def _k(name, kind, default, doc, values=None, reader="python", parse=None):
    if kind == "flag":
        values, default = _FLAG_VALUES, bool(default)
    return Knob(name, kind, default, values, reader, doc, parse or _PARSE.get(kind))


def _csrc(name, default, doc):
    return Knob(name, "csrc", default, None, "csrc", doc, None)


def _external(name, doc):
    return Knob(name, "external", None, None, "external", doc, None)


KNOBS = {k.name: k for k in (
    # ---- library and numerics
    _k("VMASR_LIB", "str", None, "path of the HIP library instead of vm_asr_amd/libvmasr_hip.so (A/B and sanitizer builds); read at import"),
    _k("VMASR_DETERMINISTIC", "flag", 0, "ordered fp32 accumulation everywhere; every stream-layout decision then keeps one stream (_lib.det_mode())"),
    _k("VMASR_LINEAR_F64ACC", "choice", "auto", "fp32 Linear with float64 accumulation: 1 always, 0 never, auto only where no gradient is recorded",
       values=("auto", "0", "1")),
    _k("VMASR_SKINNY", "choice", "1", "streaming kernel for Linear layers of many rows and few features: 1 where it beats the GEMM library, 0 off, "
       "all every supported shape", values=("1", "0", "all")),
    _k("VMASR_SPLITK_CHUNK", "int", 2048, "fewest rows of one K-split of a weight-gradient GEMM; read at import"),
    _k("VMASR_XPROJ_MAX_D", "int", 512, "largest d_inner that takes the x_proj row kernels instead of einsums; read at import"),
    # ---- generator operators (1: the HIP operator, 0: the unfused chain)
    _k("VMASR_FUSED_MLP", "flag", 1, "LayerNorm + Mlp + residual of a VSS block as one operator (mlp.py)"),
    _k("VMASR_FUSED_GMLP", "flag", 1, "LayerNorm + gated Mlp (MODEL.VSSM.GMLP) + residual of a VSS block as one operator (gmlp.py)",
       reader="python:gmlp"),
    _k("VMASR_FUSED_INPROJ", "flag", 1, "LayerNorm + in_proj + split + SiLU as one operator (inproj.py)"),
    _k("VMASR_FUSED_OUTPROJ", "flag", 1, "out_proj + DropPath + residual as one operator (outproj.py)"),
    _k("VMASR_SS2D_FUSED", "flag", 1, "the d_state-1 SS2D core (x_proj, dt_proj, four-direction scan, merge) as one operator (ss2d_core.py)"),
    _k("VMASR_SS2D_DEEP", "flag", 1, "the deep stages' SS2D core on the row-parallel kernels (ss2d_deep.py)"),
    _k("VMASR_SS2D_GLUE", "flag", 1, "the pre-scan and gated-LayerNorm glue kernels (ss2d_glue.py)"),
    _k("VMASR_SS2D_PAIRS", "flag", 1, "magnitude and phase blocks of equal shape through one gated-LayerNorm launch (ss2d_glue.py)"),
    _k("VMASR_IM2COL2D", "flag", 1, "the generator's 2-D convolutions through the row-major im2col kernel (model.py)"),
    _k("VMASR_STFT_LOSS", "flag", 1, "the multi-resolution STFT loss kernel (loss.py)"),
    _k("VMASR_LSGAN", "flag", 1, "the least-squares GAN loss kernel (loss.py)"),
    # ---- period discriminator
    _k("VMASR_MPD_BATCHED", "flag", 1, "all period discriminators layer by layer on stacked operands"),
    _k("VMASR_MPD_GEMM", "choice", "bf16x3", "fp32 discriminator GEMMs as bf16x3 MFMA triples, or fp32 library GEMMs", values=("bf16x3", "fp32")),
    _k("VMASR_MPD_CONV", "choice", None, "ONE variable read at two sites.  conv_kx1 (one discriminator at a time; unset = unfold): gemm = the "
       "im2col-free GEMM form for stride 3 and stride 1, s3 = that form for the stride-3 layers only, unfold or mfma = unfold + GEMM.  "
       "Batched path (unset = mfma): mfma = the implicit-GEMM MFMA kernels for the compute-bound layers, gemm / s3 / unfold = not those",
       values=("mfma", "gemm", "s3", "unfold")),
    _k("VMASR_MPD_CONV_L1", "choice", "f32", "the 32 -> 128 layer: f32 exact-fp32 MFMA implicit GEMM, 1 bf16x3 pairs, 0 library GEMMs",
       values=("f32", "1", "0")),
    _k("VMASR_MPD_SPLIT_MIN", "int", 1 << 18, "smallest K * N of a stacked layer that takes the split (hi, lo) GEMM path"),
    _k("VMASR_MPD_KCAT", "flag", 0, "the split GEMM's three products as one GEMM over a concatenated K"),
    _k("VMASR_MPD_FUSE_GELU_BWD", "flag", 1, "the activation backward inside the input-gradient epilogue"),
    _k("VMASR_SN_STACK", "flag", 1, "spectral normalisation, stack and permutation of a layer's weights in one launch"),
    _k("VMASR_STACK_INPUT", "flag", 1, "a layer reads the previous layer's stacked output directly"),
    _k("VMASR_CONV_POST", "flag", 1, "the 1-channel output convolution straight on the stacked maps"),
    _k("VMASR_CONV_FIRST", "flag", 1, "the 1 -> 32 channel input convolution + GELU straight from the folded signals"),
    _k("VMASR_FEAT_TAP", "flag", 1, "a feature map's gradient (next layer's + feature-matching loss's) formed in one pass"),
    _k("VMASR_FEAT_L1", "flag", 1, "the feature-matching loss on the stacked maps in one kernel"),
    # ---- scale discriminator
    _k("VMASR_MSD_CONV", "choice", "hip", "the MSD's strided grouped 1-D convolutions: hip = the exact-fp32 MFMA kernels (csrc/gconv1d.hip), "
       "torch = F.conv1d (A/B measurements, double backward)", values=("hip", "torch"), reader="python:msd"),
    _k("VMASR_MSD_STEM", "choice", "hip", "the MSD's 1 -> hidden stem convolution + GELU: hip = one fused pass that keeps no pre-activation "
       "(csrc/stem1d.hip), torch = F.conv1d + F.gelu (A/B measurements, double backward)", values=("hip", "torch"), reader="python:msd"),
    _k("VMASR_MSD_FEAT", "choice", "hip", "the MSD's feature-matching loss in the generator's pass: hip = formed on the way (the stem's share inside "
       "the stem kernels, the other maps in the one-pass L1 kernel; msd_featmatch.py), torch = forward_single + the loop of sub, abs, mean",
       values=("hip", "torch"), reader="python:msd"),
    _k("VMASR_MSD_TAIL", "choice", "torch", "the MSD's dense tail (8h -> 8h k 5 + GELU, conv_post): hip = the exact-fp32 MFMA kernels with ordered "
       "split-K sums (csrc/dconv1d.hip: bit-identical run to run, no library algorithm search), torch = F.conv1d + F.gelu (the default: "
       "faster on the 8h -> 8h layer, profiles/msd_tail.md; double backward)", values=("hip", "torch"), reader="python:msd"),
    # ---- train step
    _k("VMASR_TWO_STREAM", "choice", "1", "the discriminator on a side stream: 1 on, 0 one stream, force also in deterministic mode (test hook)",
       values=("1", "0", "force")),
    _k("VMASR_SHARE_FAKE_PASS", "flag", 1, "one discriminator pass over the fake batch serves both phases of the step"),
    _k("VMASR_GEN_STREAMS", "choice", "auto", "the generator's phase branch on a stream of its own in captured steps: auto where the trainer says so, "
       "1 off, 2 on, 2eager on in eager steps too (debugging aid)", values=("auto", "1", "2", "2eager")),
    _k("VMASR_GEN_LANES", "list", None, "comma list of the segments that leave the main stream (pe,e0..e3,d0..d3,out,ia); unset = all (dev aid)",
       parse=_comma_list),
    _k("VMASR_STEP_VARIANT", "variant", None, "pins the captured step layout: one | lane | lane:<share of the CUs for the discriminator's backward>",
       values=("one", "lane", "lane:0.75"), parse=_step_variant),
    _k("VMASR_SIDE_CUS", "int", None, "CU limit of the discriminator's convolutions beside the generator's backward (and forward unless "
       "VMASR_SIDE_CUS_FWD is set); 0 = no limit; unset = Trainer.side_cu_limits()"),
    _k("VMASR_SIDE_CUS_FWD", "int", None, "the same beside the generator's forward"),
    _k("VMASR_SIDE_CUS_MINC", "int", 0, "the backward limit only for layers at least this wide"),
    _k("VMASR_GRAPH_GC_GUARD", "flag", 1, "no cyclic garbage collection between a graph capture and its first replays"),
    _k("VMASR_PHASE_EVENTS", "flag", 0, "device-clock marks at the step's phase boundaries (tools/phase_probe.py)"),
    _k("VMASR_LN_DEFER", "flag", 1, "LayerNorm's dgamma / dbeta of a whole backward pass reduced in one launch"),
    _k("VMASR_HIP_ADAMW", "flag", 1, "the multi-tensor AdamW kernel on the flat gradient buffers"),
    _k("VMASR_FUSED_ADAMW", "flag", 1, "torch's fused AdamW where the HIP kernel does not apply"),
    _k("VMASR_HIP_SGD", "flag", 1, "the multi-tensor SGD kernel on the flat gradient buffers (TRAIN.OPTIMIZER.NAME sgd; fused_sgd.py); 0 = "
       "optimizer.step(), which graph capture refuses", reader="python:sgd"),
    _k("VMASR_LP_SHADOWS", "flag", 1, "bf16 shadow copies of the parameters, refreshed by the optimiser kernel"),
    _k("VMASR_LP_SHADOWS_T", "flag", 1, "transposed bf16 shadows of the 2-D weights too"),
    _k("VMASR_RESUME_CONFIG_MISMATCH", "choice", "raise", "a checkpoint written under another configuration: raise or warn", values=("raise", "warn")),
    # ---- distributed
    _k("VMASR_DIST_BACKEND", "str", None, "torch.distributed backend; unset = nccl on a GPU, else gloo"),
    _k("VMASR_DIST_TIMEOUT_S", "int", 600, "process-group timeout in seconds"),
    _k("VMASR_RCCL_TIMEOUT_S", "float", 300.0, "watchdog of a captured collective in seconds (rccl.py)"),
    _k("VMASR_RCCL_DIRECT", "flag", 0, "the trainer's own RCCL communicator outside captures too"),
    _k("VMASR_GRAPH_COLLECTIVES", "flag", 0, "capture the gradient all-reduces into the step's graph"),
    _k("VMASR_OVERLAP_REDUCE", "flag", 1, "asynchronous gradient all-reduces; 0 = strictly between the graphs"),
    _k("VMASR_GRAD_COMM", "choice", "fp32", "wire dtype of the gradient all-reduce: fp32, mpd-bf16 the discriminator's as bf16, bf16 both",
       values=("fp32", "mpd-bf16", "bf16")),
    _k("VMASR_GRAD_COMM_EMULATE", "choice", None, "one rank: the 16-bit wire's rounding applied to this rank's own gradient", values=("mpd-bf16", "bf16")),
    # ---- read by static getenv in vm_asr_amd/csrc
    _csrc("VMASR_CONV_CU_SLACK", 24, "convgemm.hip: CUs by which the convolution CU limit is soft"),
    _csrc("VMASR_CONV_TILE", 0, "convgemm.hip: 128 forces the small tile"),
    _csrc("VMASR_CONV_MFMA", 16, "convgemm.hip: 16 = the 16x16x32 MFMA form, 32 = 32x32x16"),
    _csrc("VMASR_CONV_F32_TILE", 128, "convgemm.hip: tile of the exact-fp32 form, 128 or 256"),
    _csrc("VMASR_XPROJ_MFMA", 0, "xproj.hip: 1 = the MFMA kernels (measured slower)"),
    _csrc("VMASR_SSCAN_N_RB", 0, "sscan_n.hip: rows per workgroup; 0 = planned"),
    _csrc("VMASR_SSCAN_N_PP", 0, "sscan_n.hip: state pairs per wave; 0 = planned"),
    _csrc("VMASR_BWD_WAVES", 0, "sscan.hip: waves of the d_state-1 backward; 0 = 8"),
    _csrc("VMASR_SSCAN_N_LEGACY", 0, "sscan.hip: non-zero = the one-state-at-a-time kernels for general d_state (A/B)"),
    # ---- owned by bench.py, tests/, oracle/
    _external("VMASR_BENCH_WATCHDOG", "bench.py: seconds after which a wedged run dumps its stacks and exits"),
    _external("VMASR_PARITY_TABLE", "tests/conftest.py: path of the achieved-error table the session writes"),
    _external("VMASR_TEST_CLIPS", "tests/test_fullsize.py: clips of the full-size accuracy test"),
    _external("VMASR_ORACLE_LIB", "oracle/oracle.py: path of the oracle library (sanitizer build)"),
    _external("VMASR_REFERENCE", "tests/golden/_refload.py: checkout of the reference project that regenerates the goldens"),
)}


def get(name):
    """The parsed value of the python-read switch `name`, from the environment as it is now."""
    k = KNOBS[name]
    raw = os.environ.get(name)
    return k.default if raw is None else k.parse(k, raw)


def undeclared():
    """VMASR_* names in the environment that no declaration covers (a misspelt switch is otherwise ignored without a word)."""
    return sorted(n for n in os.environ if n.startswith("VMASR_") and n not in KNOBS)


def warn_undeclared():
    names = undeclared()
    if names:
        warnings.warn(f"unknown VMASR_* variables in the environment (ignored): {', '.join(names)}; vm_asr_amd/knobs.py lists the switches",
                      stacklevel=2)
