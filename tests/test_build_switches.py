"""The library's behaviour depends on its documented options only: no A/B or timing-only build switch and no undocumented environment
variable in its sources.  The preprocessor may only test the acquire fallback of the persistent hand-off (RTDD_EXCHANGE_ACQUIRE, which
build() compiles and tests/test_gpu_parity.py checks bit for bit), the host / device split, the C header's own guards and -- in
sweep_diag.hpp only -- the two diagnostic hooks of the micro-benchmarks.  The one environment variable read is RTDD_DEVICE
(INTEGRATION.md).  Measured variants live in the history and EXPERIMENTS.md, not behind a -D."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "realtimedepthdiffusion_amd", "csrc")
ALLOWED = {"RTDD_EXCHANGE_ACQUIRE", "__HIPCC__", "__cplusplus", "RTDD_H"}
DIAG_ONLY = {"sweep_diag.hpp": {"RTDD_STAMPS", "RTDD_TIMELINE"}}


def _sources():
    files = [f for ext in ("hip", "cpp", "hpp", "inc") for f in glob.glob(os.path.join(CSRC, "*." + ext))]
    return sorted(files + glob.glob(os.path.join(ROOT, "include", "*")))


def test_only_the_documented_build_switches_are_tested():
    found = {}
    for path in _sources():
        name = os.path.basename(path)
        for n, line in enumerate(open(path, encoding="utf-8"), 1):
            m = re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b(.*)", line)       # every name in the condition, defined(X) included
            tested = [w for w in re.findall(r"[A-Za-z_]\w*", m.group(2).split("//")[0]) if w != "defined"] if m else []
            for macro in tested:
                if macro not in ALLOWED | DIAG_ONLY.get(name, set()):
                    found.setdefault(macro, []).append(f"{name}:{n}")
    assert not found, f"build switches outside the documented set: {found}"
    assert len(_sources()) >= 15, _sources()


def test_the_only_environment_variable_read_is_the_device():
    reads = [(os.path.basename(p), m) for p in _sources() for m in re.findall(r"\bgetenv\s*\(\s*([^)]*)\)", open(p, encoding="utf-8").read())]
    assert reads == [("dropin.cpp", '"RTDD_DEVICE"')], reads
