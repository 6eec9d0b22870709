"""The device resource layer alone (nafcodec_amd/csrc/device.cpp: DevBuf, the small-buffer cache, the stream pool) on the
CPU harness: tests/emu/device_check.cpp, a program of its own that links AddressSanitizer and UBSan itself -- a freed
buffer is poisoned memory, a kept one is not, and what is neither kept nor freed is a leak at exit."""
import os
import subprocess

from conftest import ROOT

EMU = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "nafcodec_amd", "csrc")


def test_device_resources_under_sanitizers():
    exe = os.path.join(EMU, "_build", "device_check")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Wno-unused-parameter",
                           "-DNAFGPU_EMU", "-DNAFGPU_EMU_CACHE", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",   # (the program carries its sanitizers: nothing is preloaded)
                           "-I" + EMU, "-I" + CSRC, "-o", exe, os.path.join(EMU, "device_check.cpp"),
                           os.path.join(CSRC, "device.cpp"), os.path.join(EMU, "hipemu.cpp"), "-lpthread"])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "device_check: ok" in run.stdout
