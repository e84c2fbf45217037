"""host/Service's threading under ThreadSanitizer and AddressSanitizer, on the CPU: the service is
linked against a TEST DOUBLE of the engine's C ABI (tests/support/fake_hip_engine.cc: a sentence's
"translation" is its tokens reversed, completed on a helper thread) and driven by several client
threads over two replicas with three double-buffered workers each; then the failure modes (refused
request, failing batch, workers that cannot be built, a service with none left); then every other call
kind of the service and of its C face (tests/support/service_calls.cc: score, candidates, samples,
consensus, translate with prefixes / scores / sampling / truncation beside concurrent scorers, the
refusals' exact messages), each value checked against one computed from the request alone."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "slimt_amd", "host")
SUPPORT = os.path.join(ROOT, "tests", "support")


def _build(out, sanitizer):
    srcs = [os.path.join(HOST, f) for f in ("Service.cc", "service_capi.cc", "Model.cc", "Shortlist.cc", "Io.cc")] + \
           [os.path.join(SUPPORT, f) for f in ("fake_hip_engine.cc", "service_stress.cc", "service_calls.cc")]
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", f"-fsanitize={sanitizer}", "-I", HOST,
           "-I", os.path.join(ROOT, "include")] + srcs + ["-pthread", "-o", out]
    subprocess.check_call(cmd)


@pytest.mark.parametrize("sanitizer", ["thread", "address,undefined"])
def test_service_threading_under_sanitizers(sanitizer):
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "service_stress")
        _build(exe, sanitizer)
        env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1 second_deadlock_stack=1", ASAN_OPTIONS="detect_leaks=1",
                   UBSAN_OPTIONS="halt_on_error=1")
        res = subprocess.run([exe, "4", "25"], capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "ThreadSanitizer" not in res.stderr and "AddressSanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr
    out = res.stdout
    assert " 0 wrong" in out and "rejected empty" in out and "engine failure reported" in out
    assert "survived: 2 sentences" in out
    assert "half the workers retired: 40 sentences translated" in out
    assert "dead service: " in out and "fake: out of device memory" in out
    # every other call kind (service_calls.cc): no wrong value or message, and every section ran and checked something
    assert "WRONG" not in out and "service calls: 0 wrong" in out, out
    sections = ["score (alignments 0)", "score (alignments 1)", "score_candidates (alignments 0)", "score_candidates (alignments 1)",
                "translate_samples (alignments 0)", "translate_samples (alignments 1)", "translate_consensus (alignments 0)",
                "translate_consensus (alignments 1)", "generated shortlists", "translate (prefixes, merged)",
                "translate (prefixes, one batch a launch)", "translate (sampled, merged)", "translate (sampled, one batch a launch)",
                "translate (truncated, never merged)", "C face"]
    for section in sections:
        line = next((ln for ln in out.splitlines() if ln.startswith(section + ": ")), None)
        assert line is not None, (section, out)
        assert int(line[len(section) + 2:].split()[0]) > 0, line
