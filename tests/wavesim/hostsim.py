"""TEST INFRASTRUCTURE: builds and runs the host-model programs of this directory (the kernels' sources on hip_sim.hpp, stand-alone, plain
and under ASan + UBSan / MSan).  The Makefile here holds the table of programs, their variants and every compiler flag;
this module asks it for names and binaries and holds what the tests share: the sanitizers' environment, the markers of
a report, the probe for the runtimes and the one policy for a host that lacks them.  A *_case.py next to it packs one program's input
and parses its output."""
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
BIN = os.path.join(HERE, "_build")
CXX = "/opt/rocm/lib/llvm/bin/clang++"      # the compiler of the Makefile, which holds every flag (-DTMPC_HOST_SIM and the rest)
SAN_ENV = {"ASAN_OPTIONS": "detect_stack_use_after_return=0:detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1",
           "MSAN_OPTIONS": "halt_on_error=1"}
CLEAN_MARKERS = ("ERROR: AddressSanitizer", "runtime error:", "WARNING: MemorySanitizer", "ERROR: LeakSanitizer")
SANITIZERS = {"asan": "-fsanitize=address,undefined", "msan": "-fsanitize=memory"}
_available = {}


def assert_clean(stderr):
    for m in CLEAN_MARKERS:
        assert m not in stderr, stderr[-4000:]


def sanitizers_available(tmpdir):
    """Which of asan / msan the host compiler builds and links a trivial program with (the runtimes are optional parts of a toolchain) --
    asked BEFORE a test program is built, so that a failure of the real build is a failure."""
    if not _available:
        src = os.path.join(str(tmpdir), "probe.cpp")
        with open(src, "w") as f:
            f.write("int main() { return 0; }\n")
        for kind, flag in SANITIZERS.items():
            try:
                _available[kind] = subprocess.run([CXX, flag, src, "-o", os.path.join(str(tmpdir), f"probe_{kind}")], capture_output=True).returncode == 0
            except OSError:
                _available[kind] = False
    return {k for k, ok in _available.items() if ok}


def names(program, variants=None):
    """the binaries of `program` (or of "all"): the Makefile's table, or the given variants of it ("plain", "asan", "msan", ...)"""
    if variants is not None:
        return [program if v == "plain" else f"{program}_{v}" for v in variants]
    return subprocess.run(["make", "-s", "-C", HERE, f"list-{program}"], check=True, capture_output=True, text=True).stdout.split()


def _make(want, extra):
    p = subprocess.run(["make", "-s", "-j8", "-C", HERE] + [f"_build/{n}" for n in want] + ([f"EXTRA={extra}"] if extra else []),
                       capture_output=True, text=True)
    if p.returncode != 0:
        raise RuntimeError(f"tests/wavesim: {' '.join(want)} did not build:\n{p.stderr[-8000:]}")
    return {n: os.path.join(BIN, n) for n in want}


def build(program, variants=None, extra=None):
    """make on the program's group (or on some of its variants) -> {name: path}; up to date -> no-op.  A program that does not build
    raises with the compiler's stderr."""
    return _make(names(program, variants), extra)


class _Binaries(dict):
    """{name: path}; asking for a binary that was left out for want of its sanitizer's runtime skips the test that asks"""
    lacking = {}

    def __missing__(self, name):
        if name in self.lacking:
            import pytest
            pytest.skip(f"the host toolchain ({CXX}) has no {self.lacking[name]} runtime: {name} was not built")
        raise KeyError(name)


def binaries_or_skip(tmp_path_factory, program, variants=None, extra=None, per_variant=False):
    """The one policy of the host-model tests.  A sanitizer whose runtime this host lacks: a visible skip that names it -- of every test
    of the fixture, or with per_variant of the tests that ask for a binary of that sanitizer.  A sound toolchain and a program that does
    not build: an error with the compiler's stderr.  Never an unsanitized build in a sanitized one's place."""
    have = sanitizers_available(tmp_path_factory.mktemp("sanitizer_probe"))
    lacking = {n: s for n in names(program, variants) for s in SANITIZERS if n.endswith("_" + s) and s not in have}
    if lacking and not per_variant:
        import pytest
        pytest.skip(f"the host toolchain ({CXX}) has no {', '.join(sorted(set(lacking.values())))} runtime: {' '.join(lacking)} cannot be built")
    out = _Binaries(_make([n for n in names(program, variants) if n not in lacking], extra))
    out.lacking = lacking
    return out


def run_files(binary, mode, payload, env):
    """`binary mode in out` with the arrays of payload written one after the other to `in` -> (bytes of `out`, stderr)"""
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in"), os.path.join(d, "out")
        with open(fin, "wb") as f:
            for a in payload:
                f.write(np.ascontiguousarray(a).tobytes())
        e = dict(os.environ)
        e.update(env or {})
        p = subprocess.run([binary, mode, fin, fout], capture_output=True, text=True, env=e)
        if p.returncode != 0:
            raise RuntimeError(f"{os.path.basename(binary)} {mode} failed ({p.returncode}):\n{p.stderr[-4000:]}")
        with open(fout, "rb") as f:
            raw = f.read()
    return raw, p.stderr
