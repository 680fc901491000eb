"""kernels/tile_configs.h is the one place the tile configs are written down:
the C++ side expands its X-macro lists, ops/tile_table.py parses them.  A small
driver (tests/native/tile_table_main.cpp) prints the table the preprocessor
built, looked up id by id well past both ends, under ASan + UBSan; it must be
the table the tuner uses."""
import os
import re
import shutil
import subprocess

import pytest

from rust_tensorflow_serving2_amd import ops
from rust_tensorflow_serving2_amd.ops import tile_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_preprocessor_and_python_reader_see_the_same_table(tmp_path):
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "tile_table")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I" + os.path.dirname(tile_table.HEADER), "-o", exe,
           os.path.join(ROOT, "tests", "native", "tile_table_main.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    *rows, last = r.stdout.split("\n")[:-1]
    assert last == f"igemm_configs {len(ops.TILES) - len(ops.CGEMM) - len(ops.HALO)}"
    got = {}
    for line in rows:
        cfg, fam, bm, bn = line.split()
        assert int(cfg) not in got
        got[int(cfg)] = (fam, (int(bm), int(bn)))
    assert {cfg: tile for cfg, (_, tile) in got.items()} == ops.TILES and len(got) == 93

    def ids(*families):
        return [cfg for cfg, (fam, _) in got.items() if fam in families]
    assert set(ids("cgemm", "cgemm_pf", "cgemm32", "bgemm")) == set(ops.CGEMM)
    assert ids("cgemm32") == list(ops.CGEMM32) and ids("bgemm") == list(ops.BGEMM)
    assert set(ids("halo", "halo_pf", "halo_persist")) == set(ops.HALO)
    assert ids("halo_persist") == [ops.HALO_PERSIST]
    assert set(ids("igemm")) == set(ops.TILES) - set(ops.CGEMM) - set(ops.HALO) >= ops.DMA_ONLY | set(ops.TILE_BK)
    # each PF id is a build of the tile it names
    assert len(ids("cgemm_pf")) == len(ops.CGEMM_PF_OF)
    assert [ops.CGEMM[c] for c in ids("cgemm_pf")] == [ops.CGEMM[c] for c in ops.CGEMM_PF_OF]
    assert set(ops.CGEMM_PF_OF) <= set(ids("cgemm"))


def test_a_header_that_is_missing_or_unparsable_is_an_import_error(tmp_path):
    with pytest.raises(ImportError, match="tile configs"):
        tile_table.read_rows(str(tmp_path / "nope.h"))
    bad = tmp_path / "bad.h"
    with open(tile_table.HEADER) as f:
        text = f.read()
    short = re.sub(r"X\(72,([^()]*), \d+\)", r"X(72,\1)", text)     # a row with a column missing
    assert short != text
    bad.write_text(short)
    with pytest.raises(ImportError, match="tile configs"):
        tile_table.read_rows(str(bad))
    bad.write_text("#define TFSK_IGEMM_CONFIGS(X) \\\n  X(0, 128, 128, 2, 2, 64, 0)\n")
    with pytest.raises(ImportError, match="tile configs"):
        tile_table.read_rows(str(bad))
