"""The bench's masked archive (bench.masked_leg: 40 Gbases with a Mask section, 10.2 GB) at FULL size on an MI355X (run with
-m gpu).  `bench.py` compares its decode with the checksum of the writer -- product code vouching for product code; here the
first and the last 256 Mi letters of the decode are pinned on the CPU oracle, mask included: the bit map that k_huf_decode /
k_copy_fill OR in and the run table scans at letter positions up to 4 * 10^10.

Wall time on an MI355X host, one run: 17.1 s (synthesis, write, decode, two oracle windows), next to 14.7 s for
test_both_ends_of_the_full_size_archive_against_the_oracle (tests/test_gpu_parity.py, no mask) in the same run."""
import pytest

import cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from nafcodec_amd import _ffi
    L = _ffi.default()           # raises if libnafgpu.so is missing: no CPU fallback exists
    name, hbm, cus = L.device_info(0)
    assert "gfx950" in name, name
    return L


def test_both_ends_of_the_full_size_masked_archive_against_the_oracle(lib):
    """cases.check_archive_ends(with_mask=True) on the archive of bench.masked_leg (seed 0x4E4146, 40 Gbases): the small
    archives are read by the oracle with spec_mask=True (a run cut by the window's end reaches the one record's end), the
    full archive by the product with its default, which is the same text there (tests/test_beyond_u32_emu.py asserts the
    premise on the writer's runs).  Both windows must hold lower-case letters, or nothing was compared."""
    lower = cases.check_archive_ends(lib, 40_000_000_000, 0x4E4146, 1024, with_mask=True)
    assert min(lower) > 1_000_000, lower          # a sixth of the letters is masked: 256 Mi letters hold tens of millions
