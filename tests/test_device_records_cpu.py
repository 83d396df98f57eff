"""The records the host planner uploads as raw bytes (tantivy_amd/csrc/tq_device.h), without a GPU: the device header
compiles on its own with the project's compiler and the shared intersections' per-query record keeps its 32 bytes and
its field offsets (the kernels and fill_stage agree through this layout alone)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

PROBE = r"""
#include "tq_device.h"
#include <cstddef>
#include <cstdio>
int main() {
  printf("TqdAQuery %zu %zu %zu %zu %zu %zu %zu\n", sizeof(TqdAQuery), offsetof(TqdAQuery, part_start),
         offsetof(TqdAQuery, chunk_first), offsetof(TqdAQuery, k), offsetof(TqdAQuery, term1),
         offsetof(TqdAQuery, n_terms), offsetof(TqdAQuery, ext));
  printf("TqdQuery %zu TqdALead %zu TqdLead %zu\n", sizeof(TqdQuery), sizeof(TqdALead), sizeof(TqdLead));
  return 0;
}
"""


@pytest.fixture(scope="module")
def record_sizes(tmp_path_factory):
    d = tmp_path_factory.mktemp("records")
    src = d / "records.cpp"
    src.write_text(PROBE)
    exe = str(d / "records")
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "tantivy_amd", "csrc"), str(src), "-o", exe], cwd=str(d))
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()
    return {line.split()[0]: line.split()[1:] for line in out}


def test_compact_query_record_is_32_bytes(record_sizes):
    assert [int(x) for x in record_sizes["TqdAQuery"]] == [32, 0, 4, 8, 12, 16, 20]


def test_full_records_keep_their_sizes(record_sizes):
    """328 - 32 bytes per query is what the shared intersections' group no longer uploads."""
    sizes = record_sizes["TqdQuery"]
    assert int(sizes[0]) == 328 and int(sizes[2]) == 64 and int(sizes[4]) == 128
