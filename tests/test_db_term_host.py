"""db_term_fast against db_term_spec (hpfw_amd/csrc/db_spec.h) on the host: the text the kernels compile,
run by tests/emu/db_term_check.cpp in its mode quick -- every 4099th float bit pattern from +0 to +inf, and 64 patterns
to either side of the 1e-10f clamp, of +inf, of every power of two, of the specified sequence's split at sqrt(2) and of
every cell boundary of the table in every binade.  The exhaustive mode takes a minute and a half of CPU time (11 to 17 s on eight threads) and is recorded in
tests/golden/db_term_check.json; test_gpu_db_term.py repeats it on the device."""
import pytest

import db_term_ref as ref


@pytest.fixture(scope="module")
def quick(tmp_path_factory):
    return ref.run(ref.build(tmp_path_factory), "quick")


def test_fast_equals_specified_on_the_quick_set(quick):
    print(quick)
    assert int(quick["patterns"]) == ref.INF // 4099 + 1 and int(quick["edge_patterns"]) > 2_000_000
    assert int(quick["mismatches"]) == 0, quick["first_mismatch"]


def test_fallback_stays_under_the_cap(quick):
    """over the strided sample alone (the edge patterns crowd around p = 1, where a float is finest and the fallback
    common): the share of the patterns in [1e-10f, inf), and the share of a log-uniform p in [1e-10, 1e6]"""
    print(quick)
    assert int(quick["inside"]) > 300_000 and int(quick["loguniform_patterns"]) > 100_000
    assert float(quick["fallback_share"]) <= ref.CAP
    assert float(quick["loguniform_fallback_share"]) <= ref.CAP


def test_recorded_results_belong_to_this_table(quick):
    """the exhaustive run's record (0 mismatches, the fallback count the GPU sweep is compared with) was made with the
    table, degree and delta compiled now: the quick run's figures are recorded beside it and must not have moved"""
    rec = ref.recorded()
    assert {k: quick[k] for k in rec["quick"]} == rec["quick"]
    assert {k: rec["all"][k] for k in ("cells", "degree", "delta")} == {k: quick[k] for k in ("cells", "degree", "delta")}
    assert rec["all"]["patterns"] == str(ref.INF + 1) and rec["all"]["mismatches"] == "0"
    assert int(rec["all"]["fallbacks"]) <= ref.CAP * int(rec["all"]["inside"])
    assert float(rec["all"]["loguniform_fallback_share"]) <= ref.CAP
    # delta keeps 16 times or more over the largest |y - 10 log10_spec| of any input
    assert float(rec["all"]["delta"]) >= 16 * float(rec["all"]["max_abs_diff"])


def test_quick_set_under_the_sanitizers(tmp_path_factory):
    """the same program built with -fsanitize=address,undefined (a plain host program)"""
    out = ref.run(ref.build(tmp_path_factory, sanitize=True), "quick")
    assert int(out["mismatches"]) == 0 and out["fallbacks"] == ref.recorded()["quick"]["fallbacks"]
