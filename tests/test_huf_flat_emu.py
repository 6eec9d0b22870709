"""k_huf_flat (Huffman streams of a flat tree, decoded as a gather) on the CPU harness (libnafgpu_emu.so: the same
huf_flat.hip and zplan.cpp, one fibre per work-item): hand-built frames against the CPU oracle's bytes
(tests/huf_flat_checks.py holds the checks, shared with tests/test_gpu_huf_flat.py), and the plan level and the C-ABI
under sanitizers in a program of its own (tests/huf_flat_asan_main.cpp)."""
import os
import subprocess

import pytest

import huf_flat_checks as hk
from conftest import ROOT

EMU_DIR = os.path.join(ROOT, "tests", "emu", "_build")
CSRC = os.path.join(ROOT, "nafcodec_amd", "csrc")


def make(target):
    subprocess.check_call(["make", "-s", "-C", CSRC, target], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)


@pytest.fixture(scope="module")
def emu():
    make("emu")
    from nafcodec_amd import _ffi
    return _ffi.Library(os.path.join(EMU_DIR, "libnafgpu_emu.so"))


def test_code_lengths(emu):
    hk.check_lengths(emu)


def test_sizes(emu):
    hk.check_sizes(emu)


def test_tree_reuse_mixing_and_sequences(emu):
    hk.check_mixing(emu)


def test_destination_alignment(emu):
    hk.check_fronts(emu)


def test_switch_off(emu):
    hk.check_switch_off(emu)


def test_refusals(emu):
    hk.check_refusals(emu)


def test_synthetic_archive(emu):
    hk.check_synthetic(emu, 1_000_001)          # (the harness runs a fibre per work-item: 8 M bases are the GPU test's)


def test_plan_and_c_abi_under_sanitizers(tmp_path):
    """tests/huf_flat_asan_main.cpp: pack_tasks on the frames of the checks (flat cases yield kTblFlat classes, the switch
    and the reference fixtures yield none, a plan of streams in parts is what it is with the switch off) and the frames through
    nafgpu_zstd_decompress.  `make huf-flat-asan` compiles it together with the CPU harness with
    -fsanitize=address,undefined and the sanitizer runtimes linked statically, so it runs as an ordinary child process:
    nothing is preloaded."""
    make("huf-flat-asan")
    args = hk.write_plan_inputs(str(tmp_path))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1")
    out = subprocess.run([os.path.join(EMU_DIR, "huf_flat_asan")] + args, capture_output=True, text=True, timeout=900, env=env)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-2000:] + out.stderr[-4000:]
