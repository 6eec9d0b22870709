"""Encoder(mask=True) and encode_device(mask=True) on the CPU harness (libnafgpu_emu.so: the same encode.hip / encode.cpp,
one fibre per work-item): the Mask section both encoders write, pinned on the reference's fixtures and on the run rule
(tests/mask_encode_checks.py holds the checks, shared with tests/test_gpu_mask_encode.py)."""
import os
import subprocess
import sys

import pytest

import mask_encode_checks as mc
import zstd_ref
from conftest import ROOT

EMU_DIR = os.path.join(ROOT, "tests", "emu", "_build")
CSRC = os.path.join(ROOT, "nafcodec_amd", "csrc")

pytestmark = pytest.mark.skipif(not zstd_ref.available(), reason="libzstd not loadable (tests/naf_writer.py writes the comparison archives with it)")


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-s", "-C", CSRC, "emu"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    from nafcodec_amd import _ffi
    return mc.ec.bind(_ffi.Library(os.path.join(EMU_DIR, "libnafgpu_emu.so")))


def test_the_rule_helpers_agree():
    mc.check_rule_helpers()


@pytest.mark.parametrize("name", list(mc.FIXTURES))
def test_fixture_mask_sections_are_reproduced(emu, name):
    """The Mask section written for a fixture's text decodes to the bytes `ennaf` wrote; host levels 0, 1, 3; device == host."""
    mc.check_fixture(emu, name)


HAND_MADE = mc.hand_made_cases()


@pytest.mark.parametrize("name,sequence_type,records", HAND_MADE, ids=[c[0] for c in HAND_MADE])
def test_hand_made_letters(emu, name, sequence_type, records):
    mc.check_hand_made(emu, name, sequence_type, records)


def test_masked_runs_and_record_ends(emu):
    mc.check_record_ends(emu)


def test_unaligned_device_pointer(emu):
    mc.check_unaligned_pointer(emu)


def test_errors(emu):
    mc.check_errors(emu)


CPP_PROGRAM = r"""
#include <cstdio>
#include "nafcodec.hpp"
int main() {
    using namespace nafcodec;
    Encoder enc = EncoderBuilder(SequenceType::Dna).id(true).sequence(true).compression_level(1).mask(true).with_memory();
    Record a, b;
    a.id = "r1"; a.sequence = "acGTTgcaN";
    b.id = "r2"; b.sequence = "NNacgtNN";
    enc.push(a);
    enc.push(b);
    int refused = 0;
    try { Record c; c.id = "r3"; c.sequence = "acgx"; enc.push(c); } catch (const Error &e) { refused += e.raw.status == NAFGPU_E_INVALID_SEQUENCE; }
    const std::string archive = enc.write();
    Decoder back = DecoderBuilder().with_bytes(reinterpret_cast<const uint8_t *>(archive.data()), archive.size());
    std::string text;
    while (auto rec = back.next()) text += *rec->sequence + "|";
    int invalid = 0;
    try { EncoderBuilder(SequenceType::Protein).sequence(true).mask(true).with_memory(); } catch (const Error &e) { invalid += e.raw.status == NAFGPU_E_INVALID_ARG; }
    try { EncoderBuilder(SequenceType::Dna).id(true).mask(true).with_memory(); } catch (const Error &e) { invalid += e.raw.status == NAFGPU_E_INVALID_ARG; }
    const int from_flags = EncoderBuilder::from_flags(SequenceType::Dna, Flags{0x3F}).options().mask;
    std::printf("%s refused %d invalid %d from_flags %d flag %d\n", text.c_str(), refused, invalid, from_flags, (archive[4] & 0x04) != 0);
    return 0;
}
"""


def test_cpp_encoder_builder_mask(tmp_path):
    """include/nafcodec.hpp: EncoderBuilder::mask(true), compiled and run against the CPU harness build."""
    subprocess.check_call(["make", "-s", "-C", CSRC, "emu"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    src, exe = tmp_path / "mask.cpp", tmp_path / "mask"
    src.write_text(CPP_PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", EMU_DIR, "-l:libnafgpu_emu.so", "-Wl,-rpath," + EMU_DIR])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip() == "acGTTgcaN|NNacgtNN| refused 1 invalid 2 from_flags 0 flag 1"


def test_under_address_sanitizer():
    """The mask kernels under ASan + UBSan: two fixtures, the hand-made inputs but the two largest (minutes under the
    sanitizers; they run above), the record ends, an unaligned pointer, the errors."""
    asan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not asan or not os.path.exists(asan):
        pytest.skip("libasan not available")
    subprocess.check_call(["make", "-s", "-C", CSRC, "emu-asan"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    script = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import mask_encode_checks as mc
from nafcodec_amd import _ffi
lib = mc.ec.bind(_ffi.Library(%r))
for name in ("masked", "phix"):
    mc.check_fixture(lib, name)
for case in mc.hand_made_cases():
    if case[0] not in ("case_changes_at_every_letter", "mask_section_of_several_blocks"):
        mc.check_hand_made(lib, *case)
mc.check_record_ends(lib)
mc.check_unaligned_pointer(lib)
mc.check_errors(lib)
print("OK")
""" % (ROOT, os.path.join(ROOT, "tests"), os.path.join(EMU_DIR, "libnafgpu_emu_asan.so"))
    env = dict(os.environ, LD_PRELOAD=asan, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:allocator_may_return_null=1")
    p = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=1800)
    assert p.returncode == 0 and "OK" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
