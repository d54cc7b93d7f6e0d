"""CPU tier of the row-kernel checks (tests/exact_rows.py): every case of tests/test_rows_exact_gpu.py on CPU
tensors against the fp32 torch emulation of each op, which validates each generator, each precondition (asserted
inside the cases), each float64 reference and each bound on a machine with no GPU.

And the reason for the per-element checks: each case is also run against an emulation that is wrong in one way
a row kernel could be (exact_rows.SLIPS).  The case must fail, on inputs where the whole-tensor
``rel_err < 1e-2`` of tests/test_ops_gpu.py still passes."""

import exact_rows as R
import pytest
import torch

CPU = torch.device("cpu")


@pytest.fixture(scope="module", autouse=True)
def _drop_shared_problems():
    yield
    R.clear_caches()


# ---- the comparison itself ----------------------------------------------------------------------
def test_bound_report_names_count_first_and_worst():
    ref = torch.arange(12, dtype=torch.float64).view(3, 4)
    bound = torch.full_like(ref, 0.5)
    got = ref.float().clone()
    assert R.bound_report(got, ref, bound) == (None, 0.0)
    got[1, 2] += 1
    got[2, 3] += 4
    rep, worst = R.bound_report(got, ref, bound)
    assert "2 of 12 elements over the bound" in rep and "first at (1, 2)" in rep and "worst at (2, 3)" in rep
    assert worst == 8.0
    got[0, 0] = float("nan")  # a non-finite output is a miss, never a pass
    rep, worst = R.bound_report(got, ref, bound)
    assert "3 of 12" in rep and worst == float("inf")
    rep, _ = R.bound_report(ref.float() + 1e-3, ref, torch.zeros_like(ref))  # a zero bound asks for equality
    assert "12 of 12" in rep
    assert R.bound_report(ref.float(), ref, torch.zeros_like(ref)) == (None, 0.0)


def test_exactly_zero_check():
    ck = R.Checks("zeros")
    ck.zeros("all", torch.tensor([[0.0, -0.0]]))
    ck.done()
    ck.zeros("one", torch.tensor([[0.0, 2.0**-120]]))
    with pytest.raises(AssertionError, match="1 of 2 elements are not exactly zero; first at .0, 1."):
        ck.done()


# ---- 1. LayerNorm forward -----------------------------------------------------------------------
@pytest.mark.parametrize("E", R.LN_FWD_E)
def test_ln_fwd_widths(E):
    for residual, bias in R.LN_FORMS:
        R.case_ln_fwd(CPU, 9, E, residual, bias)


@pytest.mark.parametrize("M", R.LN_FWD_M)
def test_ln_fwd_rows(M):
    for residual, bias in R.LN_FORMS:
        R.case_ln_fwd(CPU, M, 64, residual, bias)


def test_ln_fwd_offset_rows_and_view():
    R.case_ln_fwd(CPU, 9, 520, False, True, kind="offset")
    R.case_ln_fwd(CPU, 9, 520, True, True, view=True)


def test_ln_fwd_q8():
    R.case_ln_fwd_q8(CPU, 16389, 520, True, True)
    R.case_ln_fwd_q8(CPU, 21, 4104, False, False)


# ---- 2. LayerNorm backward ----------------------------------------------------------------------
@pytest.mark.parametrize("E", R.LN_BWD_FORMS_E)
def test_ln_bwd_forms(E):
    for gh, dxs in R.LN_FORMS:
        R.case_ln_bwd(CPU, 2051, E, gh, dxs)


@pytest.mark.parametrize("E", R.LN_BWD_E)
def test_ln_bwd_widths(E):
    R.case_ln_bwd(CPU, 9, E, False, False)


@pytest.mark.parametrize("M", R.LN_BWD_M)
def test_ln_bwd_rows(M):
    R.case_ln_bwd(CPU, M, 64, False, False)


@pytest.mark.parametrize("M,E", [(2051, 96), (4099, 64)])
def test_ln_bwd_accumulate(M, E):
    R.case_ln_bwd(CPU, M, E, True, True, accumulate=True)


# ---- 4. softmax and cross-entropy ---------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fused", "two_pass"])
@pytest.mark.parametrize("V", list(R.XENT_V))
def test_xent(V, mode):
    for nvalid in R.xent_nvalids(V):
        R.case_xent(CPU, V, nvalid, mode)


@pytest.mark.parametrize("scale", [1.0, 0.125])
@pytest.mark.parametrize("N", R.SOFTMAX_N)
def test_softmax(N, scale):
    R.case_softmax(CPU, N, scale)


# ---- 5. embedding -------------------------------------------------------------------------------
EMB_IDS = [(1,), (5,), (123,), (3, 41)]


@pytest.mark.parametrize("E", [8, 64, 520, 768])
def test_embedding_fwd(E):
    for shape in EMB_IDS:
        for pos in (False, True):
            R.case_embedding_fwd(CPU, E, shape, pos)


@pytest.mark.parametrize("E", [8, 64, 260, 768])
def test_embedding_bwd(E):
    if E % 8 == 0:
        R.case_embedding_bwd(CPU, E)
    R.case_embedding_bwd_acc(CPU, E)
    R.case_embedding_bwd_acc(CPU, E, deterministic=True)


# ---- each check bites: one slip each, invisible to the whole-tensor norm ------------------------
def _fails_but_norm_passes(run, names, match):
    """``run`` must fail with ``match`` in its report, while rel_err < 1e-2 holds for the outputs ``names``."""
    with pytest.raises(AssertionError, match=match):
        run()
    for n in names:
        got, ref = R.LAST[n]
        assert R.rel_err(got, ref) < 1e-2, (n, R.rel_err(got, ref))  # the old bound: blind


def test_slip_row_of_the_walk_skipped():
    be = R.Emu("row_skipped", slip_row=8195)  # the second row of wave 3
    _fails_but_norm_passes(lambda: R.case_ln_fwd(CPU, 16389, 64, False, True, be=be), ["y"],
                           r"y given the saved statistics\] 64 of 1048896 elements over the bound; first at \(8195, 0\)")


def test_slip_column_left_out_of_a_mean():
    be = R.Emu("mean_drops_column")
    _fails_but_norm_passes(lambda: R.case_ln_fwd(CPU, 9, 8192, False, True, be=be), ["y"], r"\[mean\] \d of 9 elements")


def test_slip_uncentred_variance():
    be = R.Emu("uncentred_variance")
    _fails_but_norm_passes(lambda: R.case_ln_fwd(CPU, 9, 520, False, True, kind="offset", be=be), ["y"],
                           r"\[rstd\] \d of 9 elements")
    R.case_ln_fwd(CPU, 9, 520, False, True, be=be)  # harmless on centred rows: the offset case is what catches it


def test_slip_partial_chunk_not_written():
    be = R.Emu("partial_chunk_unwritten", slip_row=2049)
    _fails_but_norm_passes(lambda: R.case_ln_bwd(CPU, 2051, 520, True, False, be=be), ["dx", "dw", "db"],
                           r"\[dx\] [1-8] of 1066520 elements over the bound; first at \(2049, 51\d\)")


def test_slip_straddling_chunk_takes_a_padded_column():
    be = R.Emu("straddle_takes_padded_column")  # the fused kernels mask per element only in that one chunk
    _fails_but_norm_passes(lambda: R.case_xent(CPU, 1024, 1021, "fused", be=be), ["grad"],
                           r"padded columns\] 4 of 15 elements are not exactly zero; first at \(0, 0\)")


def test_slip_onehot_off_by_one():
    for mode in ("fused", "two_pass"):
        be = R.Emu("onehot_off_by_one", slip_row=7)
        _fails_but_norm_passes(lambda: R.case_xent(CPU, 8, 8, mode, M=40000, be=be), ["grad"],
                               r"\[gradient\] 2 of 320000 elements over the bound; first at \(7, ")


def test_slip_local_max_rescale_dropped():
    be = R.Emu("local_max_rescale_dropped", slip_row=0)
    _fails_but_norm_passes(lambda: R.case_xent(CPU, 8200, 8197, "fused", M=1024, be=be), ["grad"],
                           r"\[gradient\] [1-8] of 8396800 elements over the bound; first at \(0, (8|9|1\d)\)")


def test_slip_partial_row_missing_from_a_column_sum():
    be = R.Emu("partial_row_missing")
    _fails_but_norm_passes(lambda: R.case_ln_bwd(CPU, 2051, 96, False, False, be=be, dy_range=(0, 8)), ["db", "dx"],
                           r"\[db\] \d+ of 96 elements differ")


def test_slip_scratch_row_left_dirty():
    be = R.Emu("scratch_row_dirty")
    _fails_but_norm_passes(lambda: R.case_embedding_bwd_acc(CPU, 64, be=be), ["gwte"],
                           r"\[call 2: gwte\] \d+ of 19200 elements differ; first at \(0, ")
    R.case_embedding_bwd_acc(CPU, 64, calls=1, be=R.Emu("scratch_row_dirty"))  # one call alone cannot see it
