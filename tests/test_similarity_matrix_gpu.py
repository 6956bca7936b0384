"""keep_similarity's dispatch table, cell by cell, against a float64 restatement of each mode.

``similarity_run`` chooses between ``sim_small_kernel`` (P <= 8, D = 768 or 1024), ``sim_mid_kernel`` (9 <= P <= 64) and the fp32 GEMM
followed by the row kernels (``row_argmax``, ``row_softmax<float>`` in place, ``row_softmax<f16>``, ``top2_partial`` / ``top2_final``).
Every cell of CELLS runs 'raw', 'argmax' (scale 25), 'softmax' (scale 10) and 'softmax_f16', plus 'top2score' where a row has a second
value (2 <= P <= 8; with one column rank_cls_score is undefined), once with the default ``sgemv_m`` and once with ``sgemv_m = 0``, which
sends every shape down the GEMM path.  Both runs are held to the same float64 reference, never to each other.

The reference is float64 numpy/torch on the host, computed from the float32 inputs the engine gets.  Row P - 1 of the bank is a copy of row
min(2, P - 2), so every cell has exact ties between two columns that live in different lanes (and, from P = 18 on, different MFMA tiles):
the engine must report the lower index, as torch.argmax does.  Where N >= 5, two tile rows lie close to that prompt (cosine 0.5), so the tie
decides rows at every P, 891 included.

Tolerances are the ones tests/test_towers_gpu.py already holds for the same quantities: raw 1e-6; scale-25 sims 3e-5; softmax 1e-6 and row
sums within 1e-5; softmax_f16 half an fp16 ulp at [0.5, 1) = 2^-12, plus the fp32 path's 1e-6; top2score 1e-6.  Labels are compared on
the rows whose float64 top-2 gap (the duplicated column left out) exceeds 1e-6 in cosine; the rows left out are asserted to be <= 1 %.
"""
import pytest
import torch

from keep_amd import KEEPModel

pytestmark = pytest.mark.gpu

F16_TOL = 2.0 ** -12 + 1e-6


def _cells():
    cells = []
    for P in (1, 2, 3, 4, 5, 7, 8):                     # sim_small, D = 768: PC = 2, 4 and 8; one row, a partial block, two blocks, many
        cells += [(P, 768, N) for N in (1, 5, 9, 1000)]
    for P in (2, 4, 8):                                 # sim_small, D = 1024 (KV = 4)
        cells += [(P, 1024, N) for N in (1, 5, 9, 1000)]
    # 3072 workgroups x 4 waves x 2 rows in flight = 24 576 rows per trip of the grid-stride loop: 24 581 starts a second trip without a
    # second row, 40 000 starts one with a second row for some waves only
    cells += [(8, 768, 24581), (8, 768, 40000)]
    for P in (9, 33, 64):                               # sim_mid off D = 768: one k block, three, sixty-four; ragged 64-row workgroups
        for D in (16, 48, 1024):
            cells += [(P, D, N) for N in (1, 63, 65, 300)]
    cells.append((4, 512, 300))                         # P <= 8 but D not in {768, 1024}: GEMM path by shape
    for P in (65, 200, 891):                            # P > 64: GEMM path by shape; row kernels with 2, 4 and 14 values per lane
        cells += [(P, 768, N) for N in (1, 5, 300)]
    cells.append((4, 768, 70000))                       # top2score: 274 block partials, so top2_final_kernel's loop takes a second trip
    return cells


CELLS = _cells()
_cache = {}


def _dup_source(P):
    return min(2, P - 2)


def make_cell(P, D, N):
    """Inputs (float32, unit rows, the tie planted) and everything the assertions need from the float64 reference.  One cell is kept:
    the two sgemv_m settings of a cell run back to back and share it; nothing in it is written after it is built."""
    key = (P, D, N)
    if _cache.get("key") == key:
        return _cache["cell"]
    g = torch.Generator().manual_seed(1000 * P + D + 7 * N)
    img = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=-1)
    txt = torch.nn.functional.normalize(torch.randn(P, D, generator=g), dim=-1)
    if P >= 2:
        txt[P - 1] = txt[_dup_source(P)]
        if N >= 5:                                      # two tiles close to the duplicated prompt: the tie decides them at every P
            w = 3 ** 0.5 if D >= 512 else 0.3           # cosine 0.5; 0.96 in 16 / 48 dimensions, where random cosines reach 0.7
            for r in (N // 2, N - 1):
                noise = torch.nn.functional.normalize(torch.randn(D, generator=g), dim=0)
                img[r] = torch.nn.functional.normalize(txt[P - 1] + w * noise, dim=0)
    ref = img.double() @ txt.double().t()                                       # [N, P] float64
    # labels: the duplicated last column can never be reported, so the decision is among the first P - 1 columns
    red = ref[:, :P - 1] if P >= 2 else ref
    exp = red.argmax(1)
    if red.shape[1] >= 2:
        top2 = red.topk(2, dim=1).values
        clear = (top2[:, 0] - top2[:, 1]) > 1e-6
    else:
        clear = torch.ones(N, dtype=torch.bool)
    tied = clear & (exp == _dup_source(P)) if P >= 2 else torch.zeros(N, dtype=torch.bool)     # rows won by the duplicated pair
    sm = torch.softmax(10.0 * ref, dim=1)
    score = None
    if 2 <= P <= 8:
        v = ref.topk(2, dim=1).values
        score = float(((v[:, 0] - v[:, 1]) - (v[:, 0] + v[:, 1] - 1).abs()).mean())
    cell = {"img": img, "txt": txt, "ref": ref, "exp": exp, "clear": clear, "tied": tied, "softmax": sm, "score": score}
    _cache["key"], _cache["cell"] = key, cell
    return cell


def check_reference_guards(P, D, N, cell):
    """Assertions on the reference alone: the label comparison leaves out at most 1 % of the rows, and where there are enough rows for
    it the planted tie decides some of them."""
    left_out = int((~cell["clear"]).sum())
    assert left_out <= 0.01 * N, f"{left_out} of {N} rows have a float64 top-2 gap below 1e-6"
    if P >= 2 and N >= 5:
        assert int(cell["tied"].sum()) >= 2, "the planted tie decides too few rows to test the tie rule"


@pytest.fixture(scope="module")
def model():
    return KEEPModel()          # the similarity kernels need no weights


@pytest.mark.parametrize("P,D,N,sgemv_m", [c + (s,) for c in CELLS for s in (16, 0)])
def test_similarity_dispatch_cell(model, P, D, N, sgemv_m):
    cell = make_cell(P, D, N)
    check_reference_guards(P, D, N, cell)
    if "img_d" not in cell:
        cell["img_d"], cell["txt_d"] = cell["img"].cuda(), cell["txt"].cuda()
    img, txt, ref = cell["img_d"], cell["txt_d"], cell["ref"]
    was = model.get_option("sgemv_m") if model._handle.value else 16.0
    assert was == 16.0
    model.set_option("sgemv_m", sgemv_m)
    try:
        raw = model.similarity(img, txt).cpu().double()
        sim, lab = model.similarity(img, txt, scale=25.0, mode="argmax")
        sim, lab = sim.cpu().double(), lab.cpu().long()
        sm = model.similarity(img, txt, scale=10.0, mode="softmax").cpu().double()
        sm16 = model.similarity(img, txt, scale=10.0, mode="softmax_f16")
        sc = model.similarity(img, txt, mode="top2score") if cell["score"] is not None else None
    finally:
        model.set_option("sgemv_m", was)
    e_raw = float((raw - ref).abs().max())
    e_sim = float((sim - 25.0 * ref).abs().max())
    e_sm = float((sm - cell["softmax"]).abs().max())
    e_sum = float((sm.sum(1) - 1).abs().max())
    e_16 = float((sm16.cpu().double() - cell["softmax"]).abs().max())
    e_sc = abs(sc - cell["score"]) if sc is not None else 0.0
    print(f"[similarity P={P} D={D} N={N} sgemv_m={sgemv_m}] raw {e_raw:.2e}  x25 {e_sim:.2e}  softmax {e_sm:.2e} (row sums {e_sum:.2e})  "
          f"f16 {e_16:.2e}  top2score {e_sc:.2e}  rows left out {int((~cell['clear']).sum())}  rows on the tie {int(cell['tied'].sum())}")
    assert raw.shape == (N, P) and e_raw < 1e-6
    assert sim.shape == (N, P) and e_sim < 3e-5
    clear, exp, tied = cell["clear"], cell["exp"], cell["tied"]
    assert lab.shape == (N,) and int(lab.min()) >= 0 and int(lab.max()) < P
    assert torch.equal(lab[clear], exp[clear])
    if P >= 2:
        assert (lab[tied] == _dup_source(P)).all() and not (lab == P - 1).any()     # the lower index of two equal columns
    assert sm.shape == (N, P) and e_sm < 1e-6 and e_sum < 1e-5
    assert sm16.dtype == torch.float16 and sm16.shape == (N, P) and e_16 < F16_TOL
    if sc is not None:
        assert e_sc < 1e-6
