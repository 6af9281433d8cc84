"""The PSIS-LOO interface on the host: include/exmc_hip_psis.h is plain C and reached through
exmc_hip_compare.h, the binding names what it declares, and its handle entry points are held to the
handle-state rules by tests/test_gpu_psis.py."""
import os
import re
import subprocess

from exmc_amd import _lib
from exmc_amd import model_comparison as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "exmc_hip_psis.h")


def _decls():
    txt = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    return re.findall(r"\b(exmc_hip_\w+)\s*\(([^)]*)\)", txt)


def test_header_is_plain_c_and_part_of_the_compare_header(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "exmc_hip_compare.h"\n'
                   'int main(void){int (*f)(exmc_hip_model*, const double*, int, int, int, size_t, double*) = '
                   'exmc_hip_psis_stats; return f != 0 && EXMC_PSIS_DEFAULT_SCRATCH != 0;}\n')
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I",
                           os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])


def test_exports_equal_the_header():
    assert sorted(_lib.PSIS_EXPORTS) == sorted({n for n, _ in _decls()})
    assert not set(_lib.PSIS_EXPORTS) & (set(_lib.EXPORTS) | set(_lib.COMPARE_EXPORTS))


def test_every_handle_entry_point_is_held_to_the_handle_state_rules():
    handle = {n for n, p in _decls() if re.search(r"\bexmc_hip_model\s*\*", p)}
    assert handle == {"exmc_hip_psis_stats", "exmc_hip_psis_stats_host"}
    txt = open(os.path.join(ROOT, "tests", "test_gpu_psis.py")).read()
    op = txt[txt.index("def op_psis("):txt.index("_fresh = {}")]
    assert '@pytest.mark.parametrize("a", list(HS.OPS))' in txt
    assert all("L.%s(" % n in op for n in handle)


def test_k_threshold():
    assert MC.k_threshold(100) == 0.5 and MC.k_threshold(10 ** 6) == 0.7
    assert abs(MC.k_threshold(2200) - 0.7) < 1e-3 and MC.k_threshold(2000) < 0.7
