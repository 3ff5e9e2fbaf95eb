"""The per-device reuse tracker behind the launch-time stream cache policy (hisparse_amd/csrc/reuse_tracker.h): plain C++, tested by a program of its
own -- nothing is loaded into python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reuse_tracker_stand_alone_under_the_sanitizers(tmp_path):
    """tests/cpp/test_reuse_tracker.cpp: cold / warm by reuse distance (A,A; A,B,A,B with 2 x 100 MB; A,B,C with 3 x 233 MB; 257 MiB), a fresh id after
    a reload, falling off the list, a forced 0 | 1, the scratch copy of a stream capture, two devices, four threads on one tracker -- compiled with
    -fsanitize=address,undefined, the runtimes linked in statically."""
    exe = tmp_path / "reuse_tracker"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", f"-I{ROOT}/hisparse_amd/csrc", f"{ROOT}/tests/cpp/test_reuse_tracker.cpp", "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "REUSE TRACKER OK" in out.stdout, out.stdout + out.stderr
