"""The device encoder on the CPU harness (libnafgpu_emu.so: the same encode.hip / encode.cpp, one fibre per work-item):
its bytes equal the host encoder's, section by section and archive by archive (tests/encode_checks.py holds the checks,
shared with tests/test_gpu_encode.py).  Both multi-chunk inputs (64 blocks + 1 byte, 129 blocks) run here: the harness
takes a few seconds for each."""
import os
import subprocess
import sys

import pytest

import encode_checks as ec
import zstd_ref
from conftest import ROOT

EMU_DIR = os.path.join(ROOT, "tests", "emu", "_build")
CSRC = os.path.join(ROOT, "nafcodec_amd", "csrc")

pytestmark = pytest.mark.skipif(not zstd_ref.available(), reason="libzstd not loadable (the frames are read back with it)")


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-s", "-C", CSRC, "emu"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    from nafcodec_amd import _ffi
    return ec.bind(_ffi.Library(os.path.join(EMU_DIR, "libnafgpu_emu.so")))


SECTION_INPUTS = ec.section_inputs() if zstd_ref.available() else []


@pytest.mark.parametrize("name,data,expect", SECTION_INPUTS, ids=[c[0] for c in SECTION_INPUTS])
def test_section_bytes_equal_the_host_encoder(emu, name, data, expect):
    """nafgpu_zstd_compress(data) is the section payload the host encoder writes; libzstd reads it back; the host frame
    takes the branch of plan_block the input was made for (block types read back out of it)."""
    ec.check_section(emu, name, data, expect)


ARCHIVES = ec.archive_cases() if zstd_ref.available() else []


@pytest.mark.parametrize("name,blob,sequence_type,fields,opts", ARCHIVES, ids=[c[0] for c in ARCHIVES])
def test_archives_equal_the_host_encoder(emu, name, blob, sequence_type, fields, opts):
    """Encoder(device=0) at levels 1 and 2 and encode_device() give the host Encoder's archive; the oracle reads it back."""
    ec.check_archive(emu, name, blob, sequence_type, fields, opts)


def test_errors(emu):
    """An invalid letter in the middle of a 1 MiB section, lengths that disagree, set_device at levels 0 and 3."""
    ec.check_errors(emu)


def test_host_path_writes_what_the_parent_commit_wrote(emu):
    """An encoder that is never given a device: two archives pinned by hashes taken from the build before this feature."""
    ec.check_host_path_unchanged(emu)


def test_slab_loop(emu, monkeypatch):
    ec.check_slabs(emu, monkeypatch)


def test_under_address_sanitizer():
    """The encode kernels under ASan + UBSan: every single-chunk section input, one archive, the error paths."""
    asan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not asan or not os.path.exists(asan):
        pytest.skip("libasan not available")
    subprocess.check_call(["make", "-s", "-C", CSRC, "emu-asan"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    script = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import encode_checks as ec
from nafcodec_amd import _ffi
lib = ec.bind(_ffi.Library(%r))
for name, data, expect in ec.section_inputs(multi_chunk=False):
    ec.check_section(lib, name, data, expect)
for case in ec.archive_cases():
    if case[0] in ("phix", "LuxC"):
        ec.check_archive(lib, *case)
ec.check_errors(lib)
print("OK")
""" % (ROOT, os.path.join(ROOT, "tests"), os.path.join(EMU_DIR, "libnafgpu_emu_asan.so"))
    env = dict(os.environ, LD_PRELOAD=asan, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:allocator_may_return_null=1")
    p = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0 and "OK" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
