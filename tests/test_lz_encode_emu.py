"""Blocks with LZ sequences from the device encoder, on the CPU harness (libnafgpu_emu.so: the same encode.hip / encode.cpp,
one fibre per work-item).  tests/lz_encode_checks.py holds the checks, shared with tests/test_gpu_lz_encode.py; the sizes and
hashes pinned there were taken here."""
import os
import subprocess
import sys

import pytest

import lz_encode_checks as lc
import zstd_ref
from conftest import ROOT

EMU_DIR = os.path.join(ROOT, "tests", "emu", "_build")
CSRC = os.path.join(ROOT, "nafcodec_amd", "csrc")

pytestmark = pytest.mark.skipif(not zstd_ref.available(), reason="libzstd not loadable (the frames are read back with it)")


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-s", "-C", CSRC, "emu"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    from nafcodec_amd import _ffi
    return lc.bind(_ffi.Library(os.path.join(EMU_DIR, "libnafgpu_emu.so")))


def test_kernel_constants():
    lc.kernel_constants()


SECTION_INPUTS = lc.section_inputs() if zstd_ref.available() else []


@pytest.mark.parametrize("name,data,check", SECTION_INPUTS, ids=[c[0] for c in SECTION_INPUTS])
def test_section(emu, name, data, check):
    """Three readers, two calls, the pinned size and hash, and the sequences read back out of the frame."""
    lc.check_section(emu, name, data, check)


SIZE_INPUTS = lc.size_inputs() if zstd_ref.available() else []


@pytest.mark.parametrize("name,data", SIZE_INPUTS, ids=[c[0] for c in SIZE_INPUTS])
def test_size_is_nearer_the_host_lz_frame_than_the_literal_only_frame(emu, name, data):
    lc.check_size(emu, name, data)


def test_nothing_to_find_gives_the_level_1_frame(emu):
    lc.check_no_repeat(emu)


def test_chunk_border(emu):
    lc.check_chunk_border(emu)


def test_slab_loop(emu, monkeypatch):
    lc.check_slabs(emu, monkeypatch)


def test_device_pointer_at_every_offset(emu):
    lc.check_device_pointer(emu)


ARCHIVES = lc.archive_cases() if zstd_ref.available() else []


@pytest.mark.parametrize("name,recs,sequence_type,fields", ARCHIVES, ids=[c[0] for c in ARCHIVES])
def test_archives(emu, name, recs, sequence_type, fields):
    """Encoder(device=0, device_lz=True) at levels 0 and 3: the oracle and Decoder read every field back; encode_device gives
    the same archive; levels 1 and 2 are today's bytes; no device: the host's bytes."""
    lc.check_archive(emu, name, recs, sequence_type, fields)


@pytest.mark.parametrize("name", sorted(lc.tc.FIXTURES))
def test_text_archives(emu, name):
    lc.check_text_archive(emu, name)


def test_refused_without_the_flag(emu):
    lc.check_refused_without_the_flag(emu)


def test_host_path_writes_what_the_parent_commit_wrote(emu):
    """literals_section now goes through plan_literals: the host's level-0 archive is the parent commit's."""
    lc.ec.check_host_path_unchanged(emu)


def test_product_launch_shape_on_the_harness():
    """The match and parse kernels with 1 024 lanes of one position, as the product launches them (`make emu-lz1024`): the pinned
    bytes of the inputs that cross tiles, segments and blocks."""
    subprocess.check_call(["make", "-s", "-C", CSRC, "emu-lz1024"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    from nafcodec_amd import _ffi
    lib = lc.bind(_ffi.Library(os.path.join(EMU_DIR, "libnafgpu_emu_lz1024.so")))
    wanted = ("64_bytes", "block_plus_1", "period_7", "period_1025", "period_70000", "match_cut_at_block_end", "ml_65539", "ll_65536",
              "dist_65533", "128_sequences", "literals_16384")
    cases = [c for c in SECTION_INPUTS if c[0] in wanted]
    assert len(cases) == len(wanted)
    for name, data, check in cases:
        lc.check_section(lib, name, data, check)


def test_under_address_sanitizer():
    """The LZ kernels under ASan + UBSan: every section input, one archive, one text archive."""
    asan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not asan or not os.path.exists(asan):
        pytest.skip("libasan not available")
    subprocess.check_call(["make", "-s", "-C", CSRC, "emu-asan"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    script = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import lz_encode_checks as lc
from nafcodec_amd import _ffi
lib = lc.bind(_ffi.Library(%r))
for name, data, check in lc.section_inputs():
    lc.check_section(lib, name, data, check)
lc.check_no_repeat(lib)
for case in lc.archive_cases():
    if case[0] in ("phix", "srr"):
        lc.check_archive(lib, *case)
lc.check_text_archive(lib, "masked")
print("OK")
""" % (ROOT, os.path.join(ROOT, "tests"), os.path.join(EMU_DIR, "libnafgpu_emu_asan.so"))
    preload = ":".join(p for p in (asan, os.environ.get("LD_PRELOAD", "")) if p)      # libasan first, nothing dropped
    env = dict(os.environ, LD_PRELOAD=preload, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:allocator_may_return_null=1")
    p = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0 and "OK" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
