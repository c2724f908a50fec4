"""glb_gemm_split_pick, the host-side choice between the split GEMM's two tile forms: a function of the
shape and the CU count alone, monotone in the row count, and consistent with the crossovers measured on the MI355X
(profiles/r28/split_gemm_forms_ab.txt: the `# crossover` lines of tools/split_gemm_ab.py --form).  No GPU."""
import ctypes as C
import os
import re

import pytest

from genlm_backend_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AB = os.path.join(ROOT, "profiles", "r28", "split_gemm_forms_ab.txt")
SERVED = ((2304, 768), (768, 768), (3072, 768), (768, 3072))
MEASURED_ROWS = (1024, 2176, 3200, 4224, 5248, 6272, 7296, 8320, 9344, 12288, 16384)
CUS = 256  # the MI355X the file was measured on


def _pick(m, n, k, cus=CUS):
    form = C.c_int(0)
    assert _lib.load().glb_gemm_split_pick(m, n, k, cus, C.byref(form)) == _lib.GLB_OK
    assert form.value in (_lib.GEMM_FORM_LARGE, _lib.GEMM_FORM_SMALL)
    return form.value


@pytest.mark.parametrize("n,k", SERVED + ((128, 64), (1024, 4096)))
@pytest.mark.parametrize("cus", (CUS, 304, 64, 1))
def test_pick_is_monotone_in_the_rows(n, k, cus):
    forms = [_pick(m, n, k, cus) for m in range(1, 20001)]
    first_large = forms.index(_lib.GEMM_FORM_LARGE) if _lib.GEMM_FORM_LARGE in forms else len(forms)
    assert all(f == _lib.GEMM_FORM_SMALL for f in forms[:first_large])
    assert all(f == _lib.GEMM_FORM_LARGE for f in forms[first_large:])


def test_pick_is_large_from_each_measured_crossover_on():
    found = {}
    for line in open(AB):
        hit = re.match(r"# crossover \S+ n (\d+) k (\d+) M (\d+|none)", line)
        if hit:
            found[(int(hit.group(1)), int(hit.group(2)))] = hit.group(3)
    assert set(found) == set(SERVED), found
    for (n, k), cross in found.items():
        if cross == "none":  # the small form won at the largest measured row count: nothing is promised
            continue
        for m in MEASURED_ROWS:
            if m >= int(cross):
                assert _pick(m, n, k) == _lib.GEMM_FORM_LARGE, (n, k, m)
        assert _pick(20000, n, k) == _lib.GEMM_FORM_LARGE


def test_pick_fills_an_empty_chip_with_the_small_form():
    # one 128 x 128 tile on 256 CUs: the launch the small form is for
    assert _pick(64, 768, 768) == _lib.GEMM_FORM_SMALL
    assert _pick(1, 128, 64) == _lib.GEMM_FORM_SMALL


def test_bad_arguments_are_refused_without_a_gpu():
    lib = _lib.load()
    form = C.c_int(0)
    assert lib.glb_gemm_split_pick(1024, 768, 768, CUS, None) == _lib.GLB_EINVAL
    for m, n, k, cus in ((0, 768, 768, CUS), (1024, 0, 768, CUS), (1024, 768, -64, CUS), (1024, 768, 768, 0)):
        assert lib.glb_gemm_split_pick(m, n, k, cus, C.byref(form)) == _lib.GLB_EINVAL
    assert lib.glb_gemm_f32_split_form(None, 0, None) == _lib.GLB_EINVAL
    a = _lib.GemmArgs()
    a.struct_size = C.sizeof(_lib.GemmArgs)
    for bad in (-1, 3, 99):
        assert lib.glb_gemm_f32_split_form(C.byref(a), bad, None) == _lib.GLB_EINVAL
        assert "form" in _lib.last_error()
    blocks = C.c_int(0)
    assert lib.glb_gemm_split_form_blocks_per_cu(0, 0, C.byref(blocks)) == _lib.GLB_EINVAL
    assert lib.glb_gemm_split_form_blocks_per_cu(_lib.GEMM_FORM_SMALL, 0, None) == _lib.GLB_EINVAL
