"""CPU: the segment plan that amx_cmllr_accumulate_dev and amx_mllr_accumulate_dev share (rasr_amd/csrc/key_plan.hpp), as a program of its
own."""
import os
import subprocess


def test_stand_alone_program_under_the_host_sanitizers(tmp_path):
    """tests/host_keyplan_test.cc: 5 segments on 3 keys (an empty segment, a key without a segment, a key's segments apart) against
    literals for key_seg, the per-key ascending order and key_base; the two early exits; every refusal's status and text under the
    caller's name.  Built with -fsanitize=address,undefined on the host side only and run as a process of its own (nothing sanitized is
    loaded into Python).  Where a GPU is present the same program is built and run plainly."""
    import torch
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "host_keyplan_test")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    sanitize = [] if torch.cuda.is_available() else ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-x", "hip", "-std=c++17", "-O1", "-g", "-w", "-ffp-contract=off"] + sanitize +
                          [os.path.join(root, "tests", "host_keyplan_test.cc"), "-o", exe])
    if sanitize:
        syms = subprocess.run(["nm", "-D", exe], capture_output=True, text=True, check=True).stdout
        assert "__asan_init" in syms and "__ubsan_handle" in syms
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "host_keyplan_test: ok" in r.stdout, r.stdout + r.stderr
