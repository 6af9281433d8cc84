"""CPU guard of the fit kernels' layout coverage: pathfinder_kernel and advi_kernel are instantiated for
every row of exmc_amd/csrc/exmc_layouts.inc, so every row of a hand-written kind is run by a Pathfinder
test and by an ADVI test (test_gpu_pathfinder.py / test_gpu_advi.py: each kind's default row;
test_gpu_fit_layouts.py: the others). A new row cannot arrive without a fit test. Also pins, from the
text of exmc_models.hpp, which models are wave-cooperative (kCoop), which the docstrings of those
tests name. Opens no library and no device."""
import os
import re

import test_gpu_advi as TA
import test_gpu_fit_layouts as FL
import test_gpu_pathfinder as TP
from test_gpu_layouts import LAYOUTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "exmc_amd", "csrc")


def layout_rows(text):
    """{(kind, lanes)} of the EXMC_LAYOUT( rows outside the EXMC_CUSTOM_HEADER block (the generated
    models' rows, whose lanes are macros of the generated header)"""
    lines = text.splitlines()
    start = lines.index("#ifdef EXMC_CUSTOM_HEADER")
    depth, end = 0, None
    for i in range(start, len(lines)):
        if re.match(r"#\s*if", lines[i]):
            depth += 1
        elif re.match(r"#\s*endif", lines[i]):
            depth -= 1
            if depth == 0:
                end = i
                break
    assert end is not None
    body = "\n".join(ln for ln in lines[:start] + lines[end + 1:] if not ln.lstrip().startswith("//"))
    rows = re.findall(r"^EXMC_LAYOUT\(\s*EXMC_MODEL_(\w+)\s*,\s*(\d+)\s*,\s*(\w+)<(\d+)>", body, flags=re.M)
    assert len(rows) == len(re.findall(r"^EXMC_LAYOUT\(", body, flags=re.M)), "a row this guard cannot read"
    assert all(lanes == g for _, lanes, _, g in rows), "a row whose model is not its lanes' instantiation"
    pairs = [(kind.lower(), int(lanes)) for kind, lanes, _, _ in rows]
    assert len(pairs) == len(set(pairs)), "a row twice"
    return set(pairs)


def coop_models(text):
    """{struct: value} for every struct of exmc_models.hpp that declares kCoop itself"""
    found, struct = {}, None
    for ln in text.splitlines():
        m = re.match(r"struct (\w+(?:<[^>]*>)?)\s*(?::|\{)", ln)
        if m:
            struct = m.group(1)
        m = re.match(r"\s*static constexpr bool kCoop = (.*);", ln)
        if m:
            assert struct is not None and struct not in found
            found[struct] = m.group(1).strip()
    return found


def _rows():
    return layout_rows(open(os.path.join(CSRC, "exmc_layouts.inc")).read())


def _run_by(module):
    """the pairs a module of default rows runs, each by a test that exists and names its lane count"""
    for (kind, lanes), name in module.FIT_LAYOUTS.items():
        assert callable(getattr(module, name)), (module.__name__, name)
        assert ("%d_lanes" % lanes) in name or (lanes == 1 and "one_lane" in name), (kind, lanes, name)
        assert lanes == LAYOUTS[kind][1][0], "the modules of default rows run default rows"
    return set(module.FIT_LAYOUTS)


def test_the_table_is_what_the_library_reports():
    rows = _rows()
    assert rows == {(kind, lanes) for kind, row in LAYOUTS.items() for lanes in row[0]}
    assert ("logistic", 4) in rows and ("eight_schools", 16) in rows and len(rows) == 15


def test_every_row_is_run_by_a_pathfinder_and_an_advi_test():
    rows = _rows()
    for module in (TP, TA):
        defaults = _run_by(module)
        assert not defaults & FL.FIT_LAYOUTS, "a row in two tables"
        assert defaults | FL.FIT_LAYOUTS == rows, (module.__name__, sorted(rows ^ (defaults | FL.FIT_LAYOUTS)))
    # the new file's tables are its parametrisations
    assert FL.FIT_LAYOUTS == ({("eight_schools", g) for g in FL.EIGHT_SCHOOLS} | set(FL.WIDE.items()) |
                              {("logistic", g) for g, _ in FL.LOGISTIC_CASES})
    for fn in (FL.test_eight_schools_pathfinder, FL.test_eight_schools_advi_mixed_convergence):
        lanes = [m.args[1] for m in fn.pytestmark if m.args[0] == "lanes"]
        assert lanes == [sorted(FL.EIGHT_SCHOOLS)]
    for fn in (FL.test_logistic_pathfinder, FL.test_logistic_advi):
        assert [m.args[1] for m in fn.pytestmark if m.name == "parametrize"] == [FL.LOGISTIC_CASES]
    for kind, lanes in FL.WIDE.items():
        for kernel in ("pathfinder", "advi"):
            assert callable(getattr(FL, "test_%s_%d_lanes_%s" % (kind, lanes, kernel)))
    # generated models: the three default layouts there, one lane with d > 2 and 32 lanes here
    for module in (TP, TA):
        (mark,) = [m for m in module.test_generated_models.pytestmark if m.name == "parametrize"]
        assert {lanes for _, lanes in mark.args[1]} == {1, 16, 64}
    assert {(name, lanes) for name, lanes, _ in FL.GENERATED_CASES} == FL.GENERATED_LAYOUTS
    assert {lanes for _, lanes in FL.GENERATED_LAYOUTS} == {1, 32}


def test_guard_sees_a_new_row_and_a_missing_case():
    text = open(os.path.join(CSRC, "exmc_layouts.inc")).read()
    more = text.replace("EXMC_LAYOUT(EXMC_MODEL_RADON, 32,",
                        "EXMC_LAYOUT(EXMC_MODEL_RADON, 16, Radon<16>, 2, rd, 0, 0, void)\n"
                        "EXMC_LAYOUT(EXMC_MODEL_RADON, 32,")
    assert layout_rows(more) - _rows() == {("radon", 16)}
    # the generated models' rows are not read
    assert not any(kind == "custom" for kind, _ in _rows())


def test_which_models_are_wave_cooperative():
    """Logistic<4>, the matrix-core model, alone among the hand-written ones; CustomSplit is the
    one-chain warmup form of a generated layout, for which no fit kernel is instantiated"""
    found = coop_models(open(os.path.join(CSRC, "exmc_models.hpp")).read())
    assert found.pop("ModelDefaults") == "false"
    assert set(found.values()) == {"true"}, "a kCoop this guard cannot read"
    assert set(found) == {"Logistic<4>", "CustomSplit"}
    assert {s for s in found if not s.startswith("Custom")} == {"Logistic<4>"}
    for module, name in ((TP, "test_logistic_pathfinder"), (TA, "test_logistic_advi")):
        doc = module.test_logistic_16_lanes_small_design.__doc__
        assert "not wave-cooperative" in doc and ("test_gpu_fit_layouts.py::" + name) in doc
