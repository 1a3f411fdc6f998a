"""The verify census on the MI355X: every instance of reference_verify_pairs_kernel<WB, Blocks, Lens> is launched on the shapes
of tests/verify_census.py — word counts 1 .. 32 at a partial and a full last word, every tail of the second column block, every
size of the last block of window rows, every window id of a five-window reference on both strands — and every distance is held
against a plain C DP on windows cut from the reference bytes on the host.  Nothing of the expectation comes from this library's
kernels.  The census's 33 words (a third column block) are named by the dispatch and refused by the calls; that refusal is
asserted here.  tests/test_verify_census_cpu.py proves on the host that the shapes reach every instance."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import bgsa_amd as B  # noqa: E402
import verify_census as C  # noqa: E402

pytestmark = pytest.mark.gpu

SENT = -77            # what an output holds where nobody may write
SPARE_OUT = 64
EUNSUPPORTED = -2


@pytest.fixture(scope="module")
def torch_gpu():
    import torch
    assert torch.cuda.is_available(), "no GPU visible"
    B.lib()
    B.check(B.lib().bgsa_hip_set_device(0), "set_device")
    return torch


def _id(x):
    return ("lens" if x else "equal") if isinstance(x, bool) else str(x)


@pytest.mark.parametrize("w,n,lens", C.cases(), ids=_id)
def test_verify_equals_the_dp(torch_gpu, w, n, lens):
    torch, L = torch_gpu, B.lib()
    c = C.case(w, n, lens)
    C.assert_worth_launching(c, w, n, lens)
    ref, m, reads = c["ref"], c["m"], c["reads"]
    windows, subjects, owned, want = c["windows"], c["subjects"], c["owned"], c["want"]
    n_pairs = windows.size
    name = L.bgsa_hip_reference_verify_kernel_name(w, int(lens)).decode()
    what = f"{w} words, {n} bp in windows of {m} bp, {name}"

    mapper = B.ReferenceMapper(np.array(ref), m, C.STRIDE)                               # the case's arrays are read-only
    a = mapper.aligner
    assert mapper.n_windows == C.N_WINDOWS and mapper.starts[-1] % C.STRIDE != 0
    assert [int(s) for s in mapper.starts] == [C.M.window_start(ref.size, m, C.STRIDE, i) for i in range(C.N_WINDOWS)]
    d_windows = torch.tensor(windows, device="cuda")
    d_subjects = torch.tensor(C.device_subjects(subjects), device="cuda")
    need = int(L.bgsa_hip_reference_verify_workspace_bytes(m, n, n_pairs))
    one_wave = int(L.bgsa_hip_reference_verify_workspace_bytes(m, n, 0))
    assert (need > 0) == (w > 16) == (one_wave > 0) and one_wave <= need
    work = torch.empty(max(need, 8), dtype=torch.uint8, device="cuda")

    def call(out, work_bytes, d_peq, d_lens, read_count):
        head = (mapper.d_reference.data_ptr(), ref.size, m, C.STRIDE, d_peq)
        tail = (n, read_count, w, d_windows.data_ptr(), d_subjects.data_ptr(), n_pairs, C.SUBJECT_BASE, out.data_ptr(),
                work.data_ptr() if need else None, work_bytes, None)
        if lens:
            return L.bgsa_hip_reference_verify_pairs_lens_dev(*head, d_lens, *tail)
        return L.bgsa_hip_reference_verify_pairs_dev(*head, *tail)

    if not C.accepted(L, w):        # 33 words: the calls launch nothing (test_verify_census_cpu.py pins which word counts these are)
        out = torch.full((n_pairs + SPARE_OUT,), SENT, dtype=torch.int32, device="cuda")
        fake = torch.zeros(64, dtype=torch.int32, device="cuda")
        assert call(out, need, fake.data_ptr(), fake.data_ptr(), 128) == EUNSUPPORTED and b"1,024" in L.bgsa_hip_last_error()
        a.check_faults()
        assert (out == SENT).all()
        return

    d_lens = None
    if lens:
        a.set_reads_ragged(reads, qlen=m)                                                   # ONE bucket, not binned
        if len(set(c["lengths"])) == 1:       # n = 1: set_reads_ragged of equal lengths IS set_subjects; the call still takes lengths
            assert a.d_lens is None
            d_lens = torch.full((128,), n, dtype=torch.int32, device="cuda")
        else:
            assert a.reads_ragged
            d_lens = a.d_lens
        assert d_lens.cpu().numpy().tolist() == c["lengths"] + [n] * 58                    # pad columns carry the width
    else:
        a.set_subjects(np.stack(reads), qlen=m)
    assert a.slen == n and a.wn == w and a.ns == 128

    def run(work_bytes):
        out = torch.full((n_pairs + SPARE_OUT,), SENT, dtype=torch.int32, device="cuda")
        B.check(call(out, work_bytes, a.d_peq.data_ptr(), d_lens.data_ptr() if lens else None, a.ns), "verify")
        a.check_faults()
        return out

    distance = run(need)
    got = distance.cpu().numpy().astype(np.int64)
    assert (got[n_pairs:] == SENT).all(), f"{what}: the spare tail was written"
    assert (got[:n_pairs][~owned] == SENT).all(), f"{what}: a pair nobody owns, or one without a window, was written"
    wrong = np.flatnonzero(owned & (got[:n_pairs] != want))
    print(f"{what}: {int(owned.sum())} pairs, {wrong.size} differ from the DP")
    assert wrong.size == 0, (f"{what}: {wrong.size} of {int(owned.sum())} distances differ from the DP; (pair, window id, read, read length, "
                             f"got, want) " + str([(int(p), int(windows[p]), int(subjects[p]), c["lengths"][subjects[p]], int(got[p]),
                                                    int(want[p])) for p in wrong[:8]]))
    if need:                                                                               # one wave's workspace: the list in chunks
        assert torch.equal(run(one_wave), distance), f"{what}: one wave's workspace gives another result"
