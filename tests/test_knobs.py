"""vm_asr_amd/knobs.py is the complete list of VMASR_* switches and the only reader of the python-read ones (CPU, no library)."""
import os
import re
import warnings

import pytest

from vm_asr_amd import knobs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SELF = os.path.abspath(__file__)
NAME = re.compile(r"VMASR_[A-Z0-9_]*[A-Z0-9]")
GETENV = re.compile(r'getenv\(\s*"(VMASR_[A-Z0-9_]+)"')
C_LIKE = (".c", ".cc", ".cpp", ".cu", ".h", ".hip", ".hpp")
TEXT = (".py", ".sh", ".md", ".txt") + C_LIKE

# name -> value with the variable unset, written down from the read sites of the commit before the registry existed
# (flags: `!= "1"` / `== "1"` against a default of "1" or "0"; None: the site asked whether the variable was set at all)
DEFAULTS = {
    "VMASR_LIB": None, "VMASR_DETERMINISTIC": False, "VMASR_LINEAR_F64ACC": "auto", "VMASR_SKINNY": "1", "VMASR_SPLITK_CHUNK": 2048,
    "VMASR_XPROJ_MAX_D": 512, "VMASR_FUSED_MLP": True, "VMASR_FUSED_INPROJ": True, "VMASR_FUSED_OUTPROJ": True, "VMASR_SS2D_FUSED": True,
    "VMASR_SS2D_DEEP": True, "VMASR_SS2D_GLUE": True, "VMASR_SS2D_PAIRS": True, "VMASR_IM2COL2D": True, "VMASR_STFT_LOSS": True,
    "VMASR_LSGAN": True, "VMASR_MPD_BATCHED": True, "VMASR_MPD_GEMM": "bf16x3", "VMASR_MPD_CONV": None, "VMASR_MPD_CONV_L1": "f32",
    "VMASR_MPD_SPLIT_MIN": 1 << 18, "VMASR_MPD_KCAT": False, "VMASR_MPD_FUSE_GELU_BWD": True, "VMASR_SN_STACK": True,
    "VMASR_STACK_INPUT": True, "VMASR_CONV_POST": True, "VMASR_CONV_FIRST": True, "VMASR_FEAT_TAP": True, "VMASR_FEAT_L1": True,
    "VMASR_TWO_STREAM": "1", "VMASR_SHARE_FAKE_PASS": True, "VMASR_GEN_STREAMS": "auto", "VMASR_GEN_LANES": None,
    "VMASR_STEP_VARIANT": None, "VMASR_SIDE_CUS": None, "VMASR_SIDE_CUS_FWD": None, "VMASR_SIDE_CUS_MINC": 0,
    "VMASR_GRAPH_GC_GUARD": True, "VMASR_PHASE_EVENTS": False, "VMASR_LN_DEFER": True, "VMASR_HIP_ADAMW": True, "VMASR_FUSED_ADAMW": True,
    "VMASR_LP_SHADOWS": True, "VMASR_LP_SHADOWS_T": True, "VMASR_RESUME_CONFIG_MISMATCH": "raise", "VMASR_DIST_BACKEND": None,
    "VMASR_DIST_TIMEOUT_S": 600, "VMASR_RCCL_TIMEOUT_S": 300.0, "VMASR_RCCL_DIRECT": False, "VMASR_GRAPH_COLLECTIVES": False,
    "VMASR_OVERLAP_REDUCE": True, "VMASR_GRAD_COMM": "fp32", "VMASR_GRAD_COMM_EMULATE": None,
}
# the defaults the static getenv sites of vm_asr_amd/csrc apply
CSRC_DEFAULTS = {"VMASR_CONV_CU_SLACK": 24, "VMASR_CONV_TILE": 0, "VMASR_CONV_MFMA": 16, "VMASR_CONV_F32_TILE": 128, "VMASR_XPROJ_MFMA": 0,
                 "VMASR_SSCAN_N_RB": 0, "VMASR_SSCAN_N_PP": 0, "VMASR_BWD_WAVES": 0, "VMASR_SSCAN_N_LEGACY": 0}


def _files():
    """vm_asr_amd/**/*.py, vm_asr_amd/csrc/*, bench.py, main.py, tests/*.py, tests/golden/*.py, tools/** (this file left out)."""
    out = [os.path.join(ROOT, "bench.py"), os.path.join(ROOT, "main.py")]
    for top, recurse in (("vm_asr_amd", True), ("tests", False), (os.path.join("tests", "golden"), False), ("tools", True)):
        for d, dirs, names in os.walk(os.path.join(ROOT, top)):
            if not recurse:
                dirs[:] = []
            dirs[:] = [x for x in dirs if x != "__pycache__" and not x.startswith("build")]
            only_py = not d.startswith(os.path.join(ROOT, "tools")) and os.path.basename(d) != "csrc"
            out += [os.path.join(d, n) for n in names if n.endswith(".py" if only_py else TEXT)]
    return [f for f in out if os.path.abspath(f) != SELF]


def _names_used():
    """{name: [files]}: in C-like sources only the string literals of getenv( (macros share the prefix), elsewhere every VMASR_* word."""
    used = {}
    for f in _files():
        with open(f, errors="ignore") as fh:
            text = fh.read()
        for n in (GETENV if f.endswith(C_LIKE) else NAME).findall(text):
            used.setdefault(n, []).append(os.path.relpath(f, ROOT))
    return used


@pytest.fixture
def clean_env(monkeypatch):
    for n in [n for n in os.environ if n.startswith("VMASR_")]:
        monkeypatch.delenv(n)
    return monkeypatch


def test_every_name_in_the_tree_is_declared_and_every_declaration_is_used():
    used = _names_used()
    here = os.path.join("vm_asr_amd", "knobs.py")
    missing = {n: fs[:3] for n, fs in used.items() if n not in knobs.KNOBS}
    assert not missing, f"VMASR_* names that vm_asr_amd/knobs.py does not declare: {missing}"
    unused = [n for n in knobs.KNOBS if not [f for f in used.get(n, []) if f != here]]
    assert not unused, f"declared in vm_asr_amd/knobs.py but named nowhere else: {unused}"
    csrc = {n for n, fs in used.items() if any(f.startswith(os.path.join("vm_asr_amd", "csrc")) for f in fs)}
    assert csrc == {n for n, k in knobs.KNOBS.items() if k.reader == "csrc"} == set(CSRC_DEFAULTS)
    assert {n: knobs.KNOBS[n].default for n in csrc} == CSRC_DEFAULTS


def test_only_the_registry_reads_the_environment():
    allowed = re.compile(r'os\.environ\.get\("(RANK|WORLD_SIZE|LOCAL_RANK)"')
    pkg = os.path.join(ROOT, "vm_asr_amd")
    bad = []
    for d, _, names in os.walk(pkg):
        for n in names:
            if n.endswith(".py") and n not in ("knobs.py", "hip_env.py"):
                with open(os.path.join(d, n)) as fh:
                    for i, line in enumerate(fh, 1):
                        if re.search(r"os\.environ|os\.getenv", allowed.sub("", line)):
                            bad.append(f"{n}:{i}")
    assert not bad, bad


def test_defaults_are_those_of_the_read_sites(clean_env):
    python_read = {n for n, k in knobs.KNOBS.items() if k.reader == "python"}
    assert python_read == set(DEFAULTS)
    for n, want in DEFAULTS.items():
        got = knobs.get(n)
        assert got == want and type(got) is type(want), (n, got, want)


def test_mpd_conv_has_one_declaration_and_two_defaults(clean_env):
    from vm_asr_amd import discriminator as D
    assert knobs.KNOBS["VMASR_MPD_CONV"].values == ("mfma", "gemm", "s3", "unfold")
    assert D._kx1_mode() == "unfold" and D._batched_conv_mode() == "mfma"
    for v in ("mfma", "gemm", "s3", "unfold"):
        clean_env.setenv("VMASR_MPD_CONV", v)
        assert D._kx1_mode() == v and D._batched_conv_mode() == v


@pytest.mark.parametrize("name", sorted(DEFAULTS))
def test_valid_values_parse_and_invalid_ones_raise(clean_env, name):
    k = knobs.KNOBS[name]
    samples = {"int": ("0", "7", "-3"), "float": ("0.5", "300"), "str": ("some/path", "gloo"), "list": ("e2", "pe,e0,out")}
    bad = {"flag": "on", "choice": "nonsense", "int": "1.5", "float": "fast", "variant": "two"}
    for v in k.values or samples[k.kind]:
        clean_env.setenv(name, v)
        got = knobs.get(name)
        if k.kind == "flag":
            assert got is (v == "1")
        elif k.kind == "choice":
            assert got == v
        elif k.kind in ("int", "float"):
            assert got == {"int": int, "float": float}[k.kind](v)
    if k.kind in bad:
        clean_env.setenv(name, bad[k.kind])
        with pytest.raises(ValueError, match=name) as e:
            knobs.get(name)
        assert bad[k.kind] in str(e.value)


def test_flags_take_exactly_0_and_1(clean_env):
    for v in ("off", "on", "true", "", "2", " 1"):
        clean_env.setenv("VMASR_FUSED_MLP", v)
        with pytest.raises(ValueError, match="VMASR_FUSED_MLP"):
            knobs.get("VMASR_FUSED_MLP")


def test_step_variant(clean_env):
    for raw, want in (("one", (False, None)), ("lane", (True, None)), ("lane:0.75", (True, 0.75)), ("lane:0.625", (True, 0.625)), ("", None)):
        clean_env.setenv("VMASR_STEP_VARIANT", raw)
        assert knobs.get("VMASR_STEP_VARIANT") == want
    for raw in ("two", "lane:abc", "lane:0", "lane:1.5", "lane:1", "lane:", "lane:nan", "ONE"):
        clean_env.setenv("VMASR_STEP_VARIANT", raw)
        with pytest.raises(ValueError, match="VMASR_STEP_VARIANT"):
            knobs.get("VMASR_STEP_VARIANT")


def test_reads_happen_at_call_time(clean_env):
    assert knobs.get("VMASR_SS2D_PAIRS") is True
    clean_env.setenv("VMASR_SS2D_PAIRS", "0")
    assert knobs.get("VMASR_SS2D_PAIRS") is False
    clean_env.delenv("VMASR_SS2D_PAIRS")
    assert knobs.get("VMASR_SS2D_PAIRS") is True


def test_undeclared_names_warn_once_and_external_ones_do_not(clean_env):
    clean_env.setenv("VMASR_BENCH_WATCHDOG", "500")      # external: bench.py's
    clean_env.setenv("VMASR_SSCAN_N_LEGACY", "1")        # csrc
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        knobs.warn_undeclared()
    assert not w
    clean_env.setenv("VMASR_FOO", "1")
    clean_env.setenv("VMASR_TWO_STREAMS", "0")           # the misspelling of VMASR_TWO_STREAM
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        knobs.warn_undeclared()
    assert len(w) == 1 and "VMASR_FOO" in str(w[0].message) and "VMASR_TWO_STREAMS" in str(w[0].message)
    assert "VMASR_BENCH_WATCHDOG" not in str(w[0].message)


def test_the_library_loader_is_where_undeclared_names_are_reported():
    import inspect
    from vm_asr_amd import _lib
    src = inspect.getsource(_lib.lib)
    assert src.count("knobs.warn_undeclared()") == 1 and src.index("if _lib is None") < src.index("knobs.warn_undeclared()")
