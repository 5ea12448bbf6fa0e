"""The glob matcher under AddressSanitizer + UndefinedBehaviorSanitizer (CPU only).

``make asan-glob`` (bayesian-consensus-engine_amd/csrc) builds tests/native/glob_fuzz.cpp, a
stand-alone program that includes csrc/glob_match.hpp -- the header the device kernel is built
from -- with g++ -fsanitize=address,undefined, and this test runs it directly: seeded random
programs, well-formed and malformed, over random byte strings in exactly sized heap arrays.  Any
sanitizer report fails the run (-fno-sanitize-recover, halt_on_error)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GLOB_FUZZ = os.path.join(ROOT, "bayesian-consensus-engine_amd", "lib", "asan", "glob_fuzz")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
           UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


def test_glob_matcher_under_asan_ubsan():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "bayesian-consensus-engine_amd", "csrc"), "asan-glob"],
                   check=True)
    r = subprocess.run([GLOB_FUZZ, "20000"], capture_output=True, text=True, env=ENV, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert "glob_fuzz ok" in r.stdout
