"""No entry point reads a workspace byte it has not written in the same call ("Workspace poisoning").

Every multi-kernel entry point carves its scratch from the handle's arena (``ensure_arena``), which only grows and is never cleared;
``keep_classify`` has a second buffer of the kind.  What those bytes held before a call is whatever the process ran last, so a
forgotten memset of an accumulator, a pad row masked by a multiply instead of a select (0 x NaN) or a hash slot assumed empty passes
every test that runs on a fresh handle or in one fixed order.  Here ``keep_debug_fill_workspace`` writes a word over both buffers
between calls and the outputs must not change by one bit.

One row of ROWS per arena-carving code path (every function that calls ``ensure_arena``, and ``keep_classify``).  Per row:
  1. the handle: slide and scoring entry points on a fresh weight-less ``KEEPModel()`` (the arena is what this entry point carves),
     the towers and ``classify`` on module-scoped models built as tests/test_reserve_gpu.py builds them;
  2. a warm call grows the arena (and ``cls_buf``); W = keep_workspace_bytes > 0 (a row that carves nothing does not belong here);
  3. fill 0x00000000, run, fill 0x00000000, run: the two runs are bit-equal (the run-to-run check) -- then for each other word fill,
     run, and after EVERY run keep_workspace_bytes == W (a call that regrew the arena ran on a fresh allocation and proved nothing);
  4. the outputs of every fill equal the 0x00000000 outputs through an integer view (NaNs compare too), and the 0x00000000 outputs are
     held once to the reference of the row's own GPU test at that test's bound, so that no row passes by being wrong every time.

The words: 0x00000000 the lucky case; 0x00000001 a non-zero count or flag (a denormal as a float, in range as an index); 0xFFFFFFFF NaN
as fp32 and as both fp16 halves, -1 as an int, the coordinate hash's empty key; 0x7FC00000 the canonical fp32 NaN whose fp16 halves are
NaN / +0 (a pad row half poisoned).

The two large words turn any arena word that is read as an index, offset, count or loop bound before the call wrote it into an
out-of-bounds access, so every row's host wrapper and kernels were read first.  The comment at a row names the kernel that first
writes each integer region; no region is read as an address component before it is written, so all four words run on every row.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from keep_amd import KEEPModel, _lib, wsi
from keep_amd.annotation import fill_numpy
from keep_amd.bootstrap import LDS_GROUPS, boot_confusion_numpy, boot_roc_numpy
from keep_amd.cluster import seed_numpy
from keep_amd.components import RegionTable, regions_numpy
from keep_amd.config import small_shape
from keep_amd.evaluation import roc_numpy
from keep_amd.heatmap import TileRaster, gaussian_taps, smooth_numpy, sort_numpy
from keep_amd.lesion import candidates_numpy, dist2_numpy, peaks_numpy
from keep_amd.model import _ptr, _stream
from keep_amd.morphometry import shape_numpy
from keep_amd.neighbours import knn_vote_numpy, topk_numpy
from keep_amd.outline import draw_numpy, outlines_numpy
from keep_amd.pca import PcaSums, moments_numpy
from keep_amd.preprocess import _center_crop, _resize_shorter_side, resize_bicubic_u8_numpy
from keep_amd.probe import ProbeSums, loss_grad_numpy
from keep_amd.quality import tile_quality_numpy
from keep_amd.region import TissueMask, TissueRule, TissueSegmentation, mask_grid_numpy, region_grid_numpy, tissue_mask_numpy, tissue_params
from keep_amd.synth import normalise_u8, synth_state_dict, synth_thumbnail, synth_tiles
from oracle import keep_oracle as O
from test_cluster import unit_rows
from test_cluster_gpu import seed_inputs
from test_evaluation import family_labels, family_scores
from test_evaluation_gpu import same_roc
from test_heatmap_display import bits, family, random_acc
from test_lesion_gpu import tile_raster_of
from test_neighbours_gpu import device_scores
from test_pca_gpu import CH, centre_of, feats as pca_feats, gram_reference, written
from test_probe_gpu import planted
from test_quality_gpu import cells_for, scene
from test_screening_shapes_gpu import MODE1_TOL, SCORE_TOL, emulated_mode1_scores, reference_scores, retrieval_reference, screening_inputs
from test_towers_gpu import tol

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WORDS = (0x00000000, 0x00000001, 0xFFFFFFFF, 0x7FC00000)
F16_TOL = 2.0 ** -12 + 1e-6          # tests/test_similarity_matrix_gpu.py: half an fp16 ulp at [0.5, 1) plus the fp32 path's 1e-6


# ------------------------------------------------------------------------------------------------ the protocol
def workspace(m) -> int:
    return int(_lib.load().keep_workspace_bytes(m._handle))


def fill(m, word: int) -> int:
    n = C.c_int64(-1)
    _lib.check(m._handle, _lib.load().keep_debug_fill_workspace(m._handle, word, C.byref(n), _stream(m._device)), "debug_fill_workspace")
    return int(n.value)


def as_bytes(t) -> torch.Tensor:
    """Any output (tensor, numpy array, Python number) as the bytes it is made of, on the host."""
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu()
    elif isinstance(t, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(t))
    else:
        t = torch.tensor([t], dtype=torch.float64 if isinstance(t, float) else torch.int64)
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    return t.contiguous().reshape(-1).view(torch.uint8)


def run(call):
    out = call()
    torch.cuda.synchronize()
    return out if isinstance(out, tuple) else (out,)


def same_bytes(a, b) -> bool:
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b))


def poison(m, call, check, cls_buf=False):
    """Steps 2 - 4 of the protocol for one row: ``call()`` -> a tensor or a tuple of them, ``check(outs)`` the reference comparison."""
    run(call)                                                            # the warm call
    W = workspace(m)
    assert W > 0, "this call carves nothing from the arena: the row is vacuous"
    filled = fill(m, 0)
    assert filled > W if cls_buf else filled >= W                        # the arena; on a shared model and in its own row keep_classify's buffer too
    base = run(call)
    assert workspace(m) == W
    want = [as_bytes(t) for t in base]
    fill(m, 0)
    again = [as_bytes(t) for t in run(call)]
    assert workspace(m) == W
    assert same_bytes(again, want), "two runs on a zeroed workspace differ: the call is not bit-reproducible on its own"
    check(base)
    for word in WORDS[1:]:
        assert fill(m, word) >= W
        got = [as_bytes(t) for t in run(call)]
        assert workspace(m) == W, f"the arena grew after the fill with {word:#010x}: that run proved nothing"
        differ = [i for i, (x, y) in enumerate(zip(got, want)) if x.shape != y.shape or not torch.equal(x, y)]
        assert not differ and len(got) == len(want), f"outputs {differ} depend on the workspace's old bytes (fill {word:#010x})"


def fresh(**options):
    m = KEEPModel()
    for k, v in options.items():
        m.set_option(k, v)
    m._ready_device()
    return m


def dev(a, dtype=None):
    return torch.from_numpy(np.array(a)).to(DEV, dtype)                  # a copy: shared cases are read-only


def exact(*wants):
    """-> check(outs): output i has the shape and the values of wants[i], a host array (every comparison here is of integers or of bits)."""
    def check(outs):
        assert len(outs) >= len(wants)
        for i, (t, w) in enumerate(zip(outs, wants)):
            t, w = t.cpu(), np.asarray(w)
            if t.dtype == torch.uint32:
                t, w = t.view(torch.int32), w.view(np.int32)
            assert tuple(t.shape) == w.shape and np.array_equal(t.numpy(), w), f"output {i} differs from its reference"
    return check


# ------------------------------------------------------------------------------------------------ the towers and classify
# The towers' workspace (carve_vit / carve_txt of engine.hip) holds fp32 / fp16 / MX-fp4 operand planes and the split-attention state:
# no integer region.  A graph-replayed call also stages pixels, ids, types and mask behind it: hipMemcpyAsync writes them before the
# graph runs, and a null types / mask pointer is passed on as null.  keep_classify's cls_buf: flags by top2_margin_flag_kernel (all N),
# list and count by compact_flags_kernel; gather / scatter read list[0 : count) only.
@pytest.fixture(scope="module")
def towers():
    sd = synth_state_dict(small_shape(2, 2), seed=5)
    g = torch.Generator().manual_seed(99)
    ctx = {"sd": sd, "bank": torch.nn.functional.normalize(torch.randn(64, 768, generator=g), dim=-1), "models": {}, "refs": {}}

    def model(precision):
        if precision not in ctx["models"]:
            m = KEEPModel(small_shape(2, 2), precision=precision)
            m.auto_calibrate = False
            m.trim_padding = False
            m.load_state_dict(sd, strict=True)
            ctx["models"][precision] = m.to(DEV).eval()
        return ctx["models"][precision]

    def ref(key, make):                                                  # a reference is computed once and not written afterwards
        if key not in ctx["refs"]:
            with torch.no_grad():
                ctx["refs"][key] = make()
        return ctx["refs"][key]

    ctx["model"], ctx["ref"] = model, ref
    return ctx


def prompts(P, T, lengths=None):
    g = torch.Generator().manual_seed(7 + P + T)
    ids = torch.randint(4, 30522, (P, T), generator=g, dtype=torch.int64)
    mask = torch.ones_like(ids)
    if lengths is not None:
        mask = (torch.arange(T)[None, :] < torch.tensor(lengths)[:, None]).to(torch.int64)
        ids = ids * mask
    return {"input_ids": ids, "token_type_ids": torch.zeros_like(ids), "attention_mask": mask}


def image_row(precision, B):
    def build(t):
        m = t["model"](precision)
        tiles = synth_tiles(33, seed=3)
        ref = t["ref"]("image", lambda: O.encode_image(t["sd"], tiles))[:B]
        x = tiles[:B].to(DEV)

        def check(outs):
            out = outs[0].cpu()
            assert out.shape == (B, 768)
            assert (out @ t["bank"].t() - ref @ t["bank"].t()).abs().max().item() < tol(precision)
        return m, lambda: m.encode_image(x), check, False
    return build


def image_u8_row(t):
    m = t["model"]("comp")
    g = torch.Generator().manual_seed(11)
    u8 = torch.randint(0, 256, (1, 224, 224, 3), dtype=torch.uint8, generator=g)
    ref = t["ref"]("image_u8", lambda: O.encode_image(t["sd"], normalise_u8(u8)))
    x = u8.to(DEV)

    def check(outs):
        assert (outs[0].cpu() @ t["bank"].t() - ref @ t["bank"].t()).abs().max().item() < tol("comp")
    return m, lambda: m.encode_image_uint8(x), check, False


def text_row(precision, P, T, lengths=None):
    def build(t):
        m = t["model"](precision)
        toks = prompts(P, T, lengths)
        ref = t["ref"](("text", P, T), lambda: O.encode_text(t["sd"], toks))
        td = {k: v.to(DEV) for k, v in toks.items()}

        def check(outs):
            out = outs[0].cpu()
            assert out.shape == (P, 768) and m.last_text_length == T
            assert (out @ t["bank"].t() - ref @ t["bank"].t()).abs().max().item() < tol(precision)
        return m, lambda: m.encode_text(td), check, False
    return build


def classify_row(t):
    """B = 40, eight prompts, margin 1: every tile is flagged, so gather, strict re-encode and scatter all run out of cls_buf."""
    m, strict = t["model"]("comp"), t["model"]("strict")
    x = synth_tiles(40, seed=8).to(DEV)
    bank = t["bank"][:8].to(DEV)
    ref = t["ref"]("classify", lambda: strict.encode_image(x).cpu() @ t["bank"][:8].t())

    def call():
        sim, lab, feats = m.classify(x, bank, margin=1.0, return_features=True)
        assert m.last_rechecked == 40
        return sim, lab, feats

    def check(outs):
        sim, lab = outs[0].cpu(), outs[1].cpu()
        assert (sim - ref).abs().max().item() < 2e-6                     # the bound of test_classify_edge_cases: all rows from the strict pass
        assert torch.equal(lab.long(), sim.argmax(1))
    return m, call, check, True


# ------------------------------------------------------------------------------------------------ scoring on a weight-less handle
def similarity_row(mode):
    """P = 70 > 64: the fp32 GEMM path, the only one that carves.  Logits by launch_sgemm_f32 (all N x P), the top2score block
    partials by top2_partial_kernel (every block): floats, no integer region."""
    def build(_):
        m = fresh()
        P, D, N = 70, 768, 300
        g = torch.Generator().manual_seed(1000 * P + D + 7 * N)
        img = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=-1)
        txt = torch.nn.functional.normalize(torch.randn(P, D, generator=g), dim=-1)
        ref = img.double() @ txt.double().t()
        img_d, txt_d = img.to(DEV), txt.to(DEV)
        if mode == "softmax_f16":
            want = torch.softmax(10.0 * ref, dim=1)

            def check(outs):
                assert outs[0].dtype == torch.float16 and (outs[0].cpu().double() - want).abs().max().item() < F16_TOL
            return m, lambda: m.similarity(img_d, txt_d, scale=10.0, mode="softmax_f16"), check, False
        if mode == "top2score":
            v = ref.topk(2, dim=1).values
            want = float(((v[:, 0] - v[:, 1]) - (v[:, 0] + v[:, 1] - 1).abs()).mean())

            def check(outs):
                assert abs(float(outs[0]) - want) < 1e-6
            return m, lambda: torch.tensor([m.similarity(img_d, txt_d, mode="top2score")], dtype=torch.float64), check, False
        top2 = ref.topk(2, dim=1).values                                 # argmax with out = null: the logits live in the arena
        clear = (top2[:, 0] - top2[:, 1]) > 1e-6
        assert int((~clear).sum()) <= 0.01 * N

        def call():
            amax = torch.full((N,), -1, dtype=torch.int32, device=DEV)
            m._call("similarity", _ptr(img_d), _ptr(txt_d), N, P, D, 25.0, _lib.SIM_ARGMAX, _ptr(None), _ptr(amax))
            return amax

        def check(outs):
            lab = outs[0].cpu().long()
            assert int(lab.min()) >= 0 and int(lab.max()) < P and torch.equal(lab[clear], ref.argmax(1)[clear])
        return m, call, check, False
    return build


def prompt_scores_row(mode, N, K, C_, D):
    """Fused: the operand planes by launch_quant_blockify (which zero-fills the bank's pad rows), the [2 ceil(N / 256)][kpad] partial sums
    by the GEMM's top-2 epilogue; A's pad rows are read by the MFMAs and must not reach a stored sum.  Unfused: logits by the sgemm,
    partials by group_top2_partial_kernel, sums by hipMemsetAsync.  Floats throughout, no integer region."""
    def build(_):
        m = fresh(fused_screening=mode)
        f, b = screening_inputs(N, K, C_, D, seed=N * 7 + K * 3 + C_ + D)
        ref, _ = reference_scores(f, b, K, C_)
        fd, bd = f.to(DEV), b.to(DEV)

        def call():
            out = torch.empty(K, dtype=torch.float32, device=DEV)
            m._call("prompt_scores", _ptr(fd), _ptr(bd), N, K, C_, D, _ptr(out))
            return out

        def check(outs):
            got = outs[0].cpu().double().numpy()
            err = float(np.abs(got - ref).max())
            if mode == 1 and D >= 256:                                   # the MX-fp4-compensated product: tests/test_screening_shapes_gpu.py
                assert err < MODE1_TOL and float(np.abs(got - emulated_mode1_scores(f, b, K, C_)).max()) < SCORE_TOL
            else:
                assert err < SCORE_TOL
        return m, call, check, False
    return build


def group_argmax_row(_):
    """The logits of a chunk by launch_sgemm_f32, then row_argmax over them: floats only."""
    m = fresh()
    N, K, C_, D = 5, 50, 3, 768
    g = torch.Generator().manual_seed(100 * N + C_)
    f = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=-1)
    b = torch.nn.functional.normalize(torch.randn(K * C_, D, generator=g), dim=-1)
    logits = (f.double() @ b.double().t()).view(N, K, C_)
    top2 = logits.topk(2, dim=2).values
    clear = (top2[..., 0] - top2[..., 1]) > 1e-6
    assert int((~clear).sum()) < 0.01 * clear.numel()
    fd, bd = f.to(DEV), b.to(DEV)

    def call():
        out = torch.full((N, K), -1, dtype=torch.int32, device=DEV)
        m._call("group_argmax", _ptr(fd), _ptr(bd), N, K, C_, D, _ptr(out))
        return out

    def check(outs):
        got = outs[0].cpu()
        assert torch.equal(got[clear], logits.argmax(2).to(torch.int32)[clear]) and int(got.min()) >= 0 and int(got.max()) < C_
    return m, call, check, False


def retrieval_row(targets):
    """The [chunk][N] similarities by launch_sgemm_f32; diag_rank_kernel's index is the caller's target, not an arena word."""
    def build(_):
        m = fresh()
        P, N, D = 70, 300, 32
        g = torch.Generator().manual_seed(77)
        img = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=-1)
        img[205], img[299] = img[5], img[40]                            # exact copies at a higher index count as above the target
        own = torch.arange(P)
        tgt = own if targets == "null" else (own * 67 + 123) % N
        assert targets == "null" or (not (tgt == own).any() and tgt.unique().numel() == P)
        a = torch.rand(P, 1, generator=g) * 1.2 + 0.8
        noise = torch.nn.functional.normalize(torch.randn(P, D, generator=g), dim=-1)
        txt = torch.nn.functional.normalize(img[tgt] + a * noise, dim=-1)
        rank, close = retrieval_reference(img, txt, tgt)
        assert int(close.sum()) <= 0.05 * P and (targets != "null" or (rank[5] >= 1 and rank[40] >= 1))
        img_d, txt_d = img.to(DEV), txt.to(DEV)
        tgt_d = None if targets == "null" else tgt.to(torch.int32).to(DEV)

        def call():
            out = torch.full((P,), -1, dtype=torch.int32, device=DEV)
            m._call("retrieval_rank", _ptr(txt_d), _ptr(img_d), P, N, D, _ptr(tgt_d), _ptr(out))
            return out

        def check(outs):
            assert torch.equal(outs[0].cpu().long()[~close], rank[~close])
        return m, call, check, False
    return build


def refine_row(overlap):
    """The hash table: keys by hipMemsetAsync(0xff) and first by hipMemsetAsync(0x7f) in launch_refine, before coord_insert_kernel.
    n = 257 with duplicates; the tile at (patch - 1, patch - 1) looks for the neighbour key (-1, -1)."""
    def build(_):
        m = fresh()
        n, grid, C_, patch = 257, 20, 4, 256
        gen = torch.Generator().manual_seed(3)
        cells = torch.randint(0, grid * grid, (n,), generator=gen)
        cells[0], cells[1] = 0, 0
        coords = torch.stack([(cells % grid) * patch + patch - 1, (cells // grid) * patch + patch - 1], dim=1).numpy()
        assert len(np.unique(coords, axis=0)) < n and (coords[0] == patch - 1).all()
        probs = torch.softmax(torch.randn(n, C_, generator=gen) * 3, dim=1)
        keys, mean = O.refine_mean_probs(probs, coords, patch, overlap)
        pd = probs.to(DEV)

        def check(outs):
            assert np.array_equal(outs[0].cpu().numpy(), np.array(keys)) and np.array_equal(outs[1].cpu().numpy(), mean)
        return m, lambda: wsi.refine(pd, coords, patch, overlap, model=m), check, False
    return build


def resize_crop_row(_):
    """The horizontally resized rows by resize_h_u8_kernel (every byte), read by resize_v_u8_kernel: pixels, no integer region."""
    from PIL import Image
    m = fresh()
    arr = (np.random.default_rng(2).random((2, 300, 512, 3)) * 255).astype(np.uint8)
    ref = np.stack([np.asarray(_center_crop(_resize_shorter_side(Image.fromarray(a), 224), 224)) for a in arr])
    x = dev(arr)
    return m, lambda: m.resize_crop_uint8(x), exact(ref), False


# ------------------------------------------------------------------------------------------------ slide regions, tissue, quality
def slide_region():
    """600 x 700 of tests/test_quality_gpu.py's scene with a band of plain glass (grey, saturation <= 5) for the tissue rule to drop."""
    a = scene(600, 700, 41)
    a[200:400, 100:500] = (236 + np.random.default_rng(1).integers(-2, 3, (200, 400, 1))).astype(np.uint8)
    return a


def region_grid_row(tissue):
    """65 x 77 = 5005 cells > REGION_GRID_CHUNK.  keep by region_tissue_count_kernel (every cell; not carved into use without a rule),
    counts by region_block_count_kernel (every block), offsets by region_scan_kernel."""
    def build(_):
        m = fresh()
        region = slide_region()
        want = region_grid_numpy(region, 16, 9, *tissue_params(tissue, 16))
        assert len(region_grid_numpy(region, 16, 9, 0, 0)) == 5005 and (tissue is None or 0 < len(want) < 5005)
        x = dev(region)
        return m, lambda: m.region_grid(x, 16, 9, tissue), exact(want), False
    return build


def region_grid_mask_row(_):
    """keep by tissue_grid_cells_kernel (every cell), then launch_region_compact as above."""
    m = fresh()
    g = np.random.default_rng(5)
    mask = np.kron(g.random((10, 11)) < 0.5, np.ones((4, 4), np.uint8)).astype(np.uint8)[:38, :44]
    want = mask_grid_numpy(mask, 16, 600, 700, 16, 9, (0, 0), "four_pt")
    assert 0 < len(want) < 5005
    x = dev(slide_region())
    tm = TissueMask(mask, 16, "four_pt")
    return m, lambda: m.region_grid(x, 16, 9, tm), exact(want), False


def region_patches_row(_):
    """The flag by hipMemsetAsync and region_check_cells_kernel, read back before a pixel is touched; the horizontally resized rows by
    region_resize_h_u8_kernel (patch = 256: the resize branch)."""
    m = fresh()
    region = slide_region()
    coords = torch.tensor([[0, 0], [444, 0], [3, 344], [444, 344], [201, 117]])
    want = np.stack([resize_bicubic_u8_numpy(region[y:y + 256, x:x + 256], 224, 224) for x, y in coords.tolist()])
    x = dev(region)
    return m, lambda: m.region_patches_uint8(x, coords, 256), exact(want), False


def region_quality_row(_):
    """The flag alone: hipMemsetAsync, region_check_cells_kernel, one read-back."""
    m = fresh()
    patch = 16
    H, W = 2 * patch + 5, 2 * patch + 6
    rgb = scene(H, W, 100 + patch)
    cells = cells_for(H, W, patch)
    want = tile_quality_numpy(rgb, cells, patch)
    x, c = dev(rgb), torch.from_numpy(cells)
    return m, lambda: m.region_quality(x, c, patch).table, exact(want), False


def tissue_mask_row(_):
    """close, min_hole and min_area all active at 130 x 70: the closing's byte plane by the first tissue_box_kernel (every pixel); labels
    and info by cc_init_kernel (every pixel, the 64 x 4 walk covers the image) before cc_merge / cc_find follow a label as an index."""
    m = fresh()
    thumb = synth_thumbnail(130, 70)
    p = TissueSegmentation(mthresh=3, close=3, min_hole=4, min_area=6)
    want, t = tissue_mask_numpy(thumb, p)
    assert 0 < want.sum() < want.size
    x = dev(thumb)

    def call():
        got = m.tissue_mask(x, 16, p)
        assert got.threshold == t
        return got.mask
    return m, call, exact(want), False


# ------------------------------------------------------------------------------------------------ heatmap: sort, smoothing
def sort_row(M):
    """Only the many-block path carves (M > 4096).  The keys by sort_scatter_kernel<first> (the table sums to M: every place), the digit
    table by sort_hist_kernel (all 256 nb entries), the chunk totals by sort_scan1_kernel; a place is checked against M before the store."""
    def build(_):
        m = fresh()
        v = family("seven", M)
        v[::97] = np.nan
        want, n = sort_numpy(v)
        x = dev(v)

        def call():
            ref = m.score_reference(x)
            return ref.sorted, ref.n

        def check(outs):
            assert np.array_equal(bits(outs[0].cpu().numpy()), bits(want)) and int(outs[1].item()) == n
        return m, call, check, False
    return build


def smooth_row(masked):
    """The two planes of the row pass by heat_smooth_row_kernel (every x < w of every row), read by heat_smooth_col_kernel inside the
    raster only: sums, no integer region."""
    def build(_):
        m = fresh()
        g = np.random.default_rng(130 * 1000 + 70)
        acc = random_acc(g, 130, 70)
        mask = g.random((130, 70)) < 0.75
        taps = gaussian_taps(4.7, 14)
        want = smooth_numpy(acc, taps, mask if masked else None)
        r = TileRaster(dev(acc), 16, 224, model=m)
        tissue = TissueMask(mask, 16) if masked else None
        return m, lambda: m.smooth_raster(r, taps=taps, tissue=tissue).acc, exact(want), False
    return build


# ------------------------------------------------------------------------------------------------ regions, outlines, shape, polygons
def label_case():
    """67 x 129 = 8643 pixels: five blocks of every 2048-wide scan."""
    g = np.random.default_rng(67 + 129)
    img = np.kron(g.random((67 // 9 + 1, 129 // 13 + 1)) < 0.6, np.ones((9, 13), np.uint8))[:67, :129].astype(np.uint8)
    img[67 // 3:67 // 3 + 40, 129 // 4:129 // 4 + 50] = 1
    img[g.random(img.shape) < 0.03] ^= 1                                  # specks and pin holes: small regions, holes
    return img


def regions_label_row(min_area):
    """roots and info by cc_init_kernel (every pixel) before any label is followed; counts by regions_root_count_kernel, offsets by
    regions_scan_kernel; regions_relabel_kernel indexes info by a root, which is a pixel index < n."""
    def build(_):
        m = fresh()
        img = label_case()
        labels, table = regions_numpy(img, 8, min_area)
        assert len(table) >= 2 and (min_area == 1 or len(table) < len(regions_numpy(img, 8, 1)[1]))      # regions are dropped at min_area > 1
        x = dev(img)

        def call():
            regs = m.mask_regions(x, 8, min_area)
            return regs.labels, regs.table
        return m, call, exact(labels, table), False
    return build


def outlines_row(_):
    """keep_outline_count: counts by outline_count_kernel (every block).  keep_outline_trace: flags by hipMemsetAsync; counts / offsets by
    outline_count / outline_scan; pixoff (every pixel) and slot (every edge) by outline_compact_kernel; succ and state 0 by
    outline_succ_kernel; state k by round k, and outline_pick names a state whose round ran; lead / a0 / w0 by outline_rank_init_kernel;
    start_of by outline_rings_kernel for every leader.  Every index read from the arena is a successor or leader < E or guarded."""
    m = fresh()
    labels, table = regions_numpy(label_case(), 8, 1)
    n = len(table)
    rings, vertices = outlines_numpy(labels, 8, n)
    assert len(rings) > n                                                # holes among them
    lab = dev(labels)

    def call():
        o = m.region_outlines(lab, 8, n=n)
        return o.rings, o.vertices
    return m, call, exact(rings, vertices), False


def outline_draw_row(_):
    """rowok by outline_draw_rows_kernel (every pixel), read by outline_draw_kernel: bytes, no index."""
    m = fresh()
    labels, _ = regions_numpy(label_case(), 4, 1)
    rgb = np.random.default_rng(3).integers(0, 256, labels.shape + (3,), dtype=np.uint8)
    want = draw_numpy(rgb, labels, (255, 0, 128), 3)
    lab, x = dev(labels), dev(rgb)
    return m, lambda: m.draw_outlines(x, lab, (255, 0, 128), 3), exact(want), False


def region_shape_row(_):
    """Both carve sites of keep_regions_feret: the plan (line_off, wg_off, totals: feret_plan_kernel, every entry) and, after the
    read-back of the totals, the lines (feret_init_kernel, every entry) that feret_lines_kernel then narrows with atomics."""
    m = fresh()
    labels, table = regions_numpy(label_case(), 8, 1)
    moments, feret = shape_numpy(labels, table, True)
    regs = RegionTable(dev(table), dev(labels))

    def call():
        sh = m.region_shape(regs)
        return sh.moments, sh.feret
    return m, call, exact(moments, feret), False


def poly_fill_row(rule, with_into):
    """4 x 4099: a row wider than PF_ROW_CHUNK; one ring per set pixel, V > POLY_CHUNK.  delta by hipMemsetAsync; info and off (every
    vertex) and sums by poly_edges_kernel; boff and the total by poly_scan_kernel; poly_crossings_kernel's searches run over them."""
    def build(_):
        m = fresh()
        h, w, d = 4, 4099, 3
        g = np.random.default_rng(h * 7 + w)
        img = (g.random((h, w)) < 0.5).astype(np.uint8)
        ys, xs = np.nonzero(img)
        corners = np.array([(0, 0), (1, 0), (1, 1), (0, 1)], np.int64)
        vertices = ((np.stack([xs, ys], 1)[:, None, :] + corners[None]) * d).reshape(-1, 2).astype(np.int64)
        start = np.arange(0, 4 * len(xs) + 1, 4, dtype=np.int64)
        weight = np.ones(len(xs), np.int32)
        assert len(vertices) > 2048
        into = g.integers(0, 256, (h, w), dtype=np.uint8) if with_into else None
        want = fill_numpy((vertices, start, weight), d, (h, w), rule=rule, value=7, into=into)
        assert np.array_equal(want == 7, (img != 0) | (False if into is None else into == 7))
        polys = (vertices, start, weight)
        into_d = None if into is None else dev(into)
        return m, lambda: m.fill_polygons(polys, d, (h, w), rule=rule, value=7, into=into_d), exact(want), False
    return build


# ------------------------------------------------------------------------------------------------ evaluation, bootstrap, lesions
def eval_roc_row(curve):
    """N = 4097 with ties and NaNs (the sort's many-block path twice).  sp / sn by roc_split_kernel, the counts by the sort, flags by
    hipMemsetAsync, totals by ev_scan1_kernel, the candidates by roc_best_kernel; without the caller's curve the curve lives in the
    arena too and roc_points_kernel<emit> writes every k < K of it.  Every count read from the arena is clamped (ev_count)."""
    def build(_):
        m = fresh()
        n = 4097
        g = np.random.default_rng(n + 1)
        s = family_scores("three_ints", n, g) - 1
        s[g.random(n) < 0.2] = np.nan
        s[g.random(n) < 0.2] = -0.0
        s[:4] = [0.0, -0.0, -1.0, 1.0]
        y = family_labels("informative", np.nan_to_num(s), g)
        y[:4] = [1, 0, 0, 1]
        want = roc_numpy(s, y)
        assert want.n < n
        sd_, yd = dev(s), dev(y)
        state = {}

        def call():
            r = state["roc"] = m.tile_roc(sd_, yd, curve=curve)
            scalars = torch.tensor([r.n, r.n_pos, r.n_neg, r.u2], dtype=torch.int64)
            best = torch.tensor([r.best_threshold], dtype=torch.float64)
            return (scalars, best, r.thresholds, r.fps, r.tps, r.kept) if curve else (scalars, best)

        def check(outs):
            assert same_roc(state["roc"], want, curve)
        return m, call, check, False
    return build


def boot_roc_row(kind):
    """sorted / n by the sort, both flag arrays (padded to whole chunks) by boot_flags_kernel, totals by boot_scan1_kernel, meta by
    boot_scan2_kernel, items[0 : n) by boot_items_kernel; with K > BOOT_LDS_GROUPS a workgroup zeroes its global slab before it adds.
    boot_roc_kernel clamps meta and tests every item word against the bin count."""
    def build(_):
        m = fresh()
        n, B = (LDS_GROUPS + 1, 3) if kind == "slabs" else (300, 5)
        g = np.random.default_rng(n)
        y = (g.random(n) < 0.25).astype(np.uint8)
        y[:2] = [1, 0]
        if kind == "slabs":
            s = (g.permutation(n) / n).astype(np.float32)               # all distinct: K = N = 8193 > 8192
            assert len(np.unique(s)) == n
        else:
            s = (np.round(g.random(n) * 16) / 4 - 2).astype(np.float32)
            s[[7, 70, 130, 200]] = np.nan
        want = boot_roc_numpy(s, y, B + 1, 11, first_replicate=-1)
        sd_, yd = dev(s), dev(y)
        return m, lambda: m.bootstrap_roc(sd_, yd, n_boot=B, seed=11)[0], exact(want[1:]), False
    return build


def boot_confusion_row(C_):
    """The code bytes by boot_codes_kernel (every item); the tables live in LDS."""
    def build(_):
        m = fresh()
        n, B = 300, 8
        g = np.random.default_rng(n + C_)
        t = g.integers(0, C_, n).astype(np.uint8)
        p = np.where(g.random(n) < 0.7, t, g.integers(0, C_, n)).astype(np.uint8)
        want = boot_confusion_numpy(t, p, C_, B + 1, 11, first_replicate=-1)
        return m, lambda: m.bootstrap_confusion(t, p, C_, n_boot=B, seed=11), exact(want[1:]), False
    return build


def mask_dist2_row(to):
    """The uint16 plane of the column pass by dist_cols_kernel (every pixel of every band), read by dist_rows_kernel: distances."""
    def build(_):
        m = fresh()
        mask = (np.random.default_rng(67 + 129).random((67, 129)) < 0.02).astype(np.uint8)
        want = dist2_numpy(mask, 64, to)
        md = dev(mask)
        return m, lambda: m.mask_distance(md, 64, to), exact(want), False
    return build


def raster_peaks_row(masked):
    """rowmax by peak_rows_kernel (every pixel), counts by peak_cols_kernel<count> (every block), offsets by peak_scan_kernel; a peak's
    row in the output is tested against max_peaks."""
    def build(_):
        m = fresh()
        shape = (67, 129)
        g = np.random.default_rng(shape[0] * 7 + shape[1])
        raster = tile_raster_of(m, shape, g)                             # keep_heat_accumulate: no workspace
        acc = raster.acc.cpu().numpy()
        tissue = (g.random(shape) < 0.7).astype(np.uint8)
        want = candidates_numpy(peaks_numpy(acc, 2, 0, tissue if masked else None), raster.downsample, raster.origin)
        assert len(want.xy) > 5
        tm = TissueMask(tissue, raster.downsample) if masked else None

        def call():
            got = m.raster_peaks(raster, 2, 0.0, tm)
            return got.xy, got.scores, got.m16
        return m, call, exact(want.xy, want.scores, want.m16), False
    return build


# ------------------------------------------------------------------------------------------------ clustering, probe, PCA, neighbours
def cluster_seed_row(_):
    """The 64-bit key by hipMemsetAsync(0xFF) in launch_cluster_seed_step.  A NaN row is skipped."""
    m = fresh()
    x, k = seed_inputs("blobs")
    want = seed_numpy(x, k)
    xd = dev(x)
    return m, lambda: m.cluster_seed(xd, k, normalize=False), exact(want), False


def probe_row(_):
    """The flag alone: hipMemsetAsync, probe_check_kernel, one read-back.  A NaN row and two unlabelled rows are skipped."""
    m = fresh()
    D, C_, N = 768, 17, 65
    x, y, w, b, cw = planted(D, C_, N, 0)
    xd, yd, wd, bd, cwd = dev(x), dev(y), dev(w), dev(b), dev(cw)

    def call():
        sums = ProbeSums(C_, D, DEV)
        labels, probs, best, margin = m.probe_loss_grad(xd, yd, wd, bd, sums, class_weight=cwd, normalize=False, forward=True)
        return sums.buf, labels, probs, best, margin

    def check(outs):
        got = ProbeSums(C_, D)
        got.buf.copy_(outs[0].cpu())
        got, want = got.host(), loss_grad_numpy(x, y, outs[2].cpu().numpy(), cw)
        assert np.array_equal(got["grad"], want["grad"]) and np.array_equal(got["gbias"], want["gbias"])
        assert np.array_equal(got["counts"], want["counts"]) and got["skipped"] == want["skipped"] == 2
    return m, call, check, False


def pca_row(_):
    """The kept bytes by pca_sums_kernel (every row), read by pca_gram_kernel.  Four rows are skipped; 2 chunks + 37 rows."""
    m = fresh()
    n, d = 2 * CH + 37, 48
    c = centre_of(d)
    x = np.array(pca_feats(n, d))
    for r, v in zip([0, CH - 1, CH, n - 1], (np.nan, np.inf, 1.5, -np.inf)):
        x[r, (7 * r) % d] = v
    s, _, cnt, skp = moments_numpy(x, c, CH)
    ref, bound = gram_reference(x, c)
    xd = dev(x)

    def call():
        sums = PcaSums(d, c, DEV)
        m.pca_moments(xd, sums, normalize=False)
        return sums.buf, sums.sum, sums.gram, sums.count, sums.skipped

    def check(outs):
        assert torch.equal(outs[1].cpu(), torch.from_numpy(s)) and (int(outs[3]), int(outs[4])) == (cnt, skp) == (n - 4, 4)
        wr = written(d)
        assert (np.abs(outs[2].cpu().numpy() / 2.0 ** 32 - ref)[wr] <= bound[wr]).all()
    return m, call, check, False


def neighbour_case():
    D, M, Nq, k = 32, 200, 20, 20
    q, b = unit_rows(Nq, D, 300 + M).copy(), unit_rows(M, D, 400 + Nq).copy()
    clean = device_scores(fresh(), q, b)                                 # every score as the device computes it, one small call per 64 bank rows
    q[7, 5] = np.nan
    b[0, 3], b[63, 31], b[64, 0] = np.nan, np.inf, 1.5
    want = clean.copy()
    want[:, [0, 63, 64]] = np.nan
    want[7] = np.nan
    return q, b, k, topk_numpy(want, k)


def topk_row(_):
    """Three bank segments, so that the merge runs: every (segment, query block) writes its 64 lists into the arena from LDS lists that
    start at zero, and topk_merge_kernel reads those.  Keys, no integer region.  A NaN query and three bad bank rows are skipped."""
    m = fresh()
    q, b, k, want = neighbour_case()
    qd, bd = dev(q), dev(b)

    def call():
        nb = m.topk(qd, bd, k, normalize=False, segments=3)
        return nb.keys, nb.index, nb.score, nb.count, nb.query_skipped, nb.bank_skipped

    def check(outs):
        assert np.array_equal(outs[0].cpu().numpy().view(np.uint64), want) and int(outs[4]) == 1 and int(outs[5]) == 3
    return m, call, check, False


def knn_vote_row(_):
    """The flag alone: hipMemsetAsync, knn_check_kernel, one read-back.  Query 7 has no neighbour and is skipped."""
    m = fresh()
    q, b, k, want = neighbour_case()
    nb = fresh().topk(dev(q), dev(b), k, normalize=False)                # another handle makes the lists: this row's arena is the vote's alone
    idx, sc = nb.index.cpu().numpy(), nb.score.cpu().numpy()
    labels = np.random.default_rng(3).integers(-1, 3, 200).astype(np.int32)
    wl, wp, wm, ws = knn_vote_numpy(idx, sc, labels, 3, "uniform")
    assert wl[7] == -1 and ws >= 1

    def check(outs):
        assert np.array_equal(outs[0].cpu().numpy(), wl) and np.array_equal(outs[1].cpu().numpy(), wp)
        assert np.array_equal(outs[2].cpu().numpy(), wm) and int(outs[3]) == ws
    return m, lambda: m.knn_vote(nb, labels, 3, weights="uniform"), check, False


# ------------------------------------------------------------------------------------------------ the table
ROWS = {}
for _p in ("comp", "strict", "fp16"):
    for _B in (1, 6, 33):                        # graph-replayed (197 rows in a 256-row plane); the first size that is not; a ragged second lane
        ROWS[f"encode_image-{_p}-{_B}"] = image_row(_p, _B)
ROWS["encode_image_uint8-1"] = image_u8_row
for _p in ("comp", "strict"):
    ROWS[f"encode_text-{_p}-1x8"] = text_row(_p, 1, 8)
    ROWS[f"encode_text-{_p}-3x40-masked"] = text_row(_p, 3, 40, [40, 17, 5])
    ROWS[f"encode_text-{_p}-2x300"] = text_row(_p, 2, 300)            # the two key windows of split attention
ROWS["classify-40"] = classify_row
for _mode in ("softmax_f16", "top2score", "argmax_no_out"):
    ROWS[f"similarity-{_mode}"] = similarity_row(_mode)
for _mode in (1, 2):
    ROWS[f"prompt_scores-fused{_mode}-130x65"] = prompt_scores_row(_mode, 130, 65, 4, 768)     # A pad rows 130..255, bank pad rows 260..511, two row slots
    ROWS[f"prompt_scores-fused{_mode}-257x64"] = prompt_scores_row(_mode, 257, 64, 4, 768)     # a second row tile holding one valid row
ROWS["prompt_scores-unfused-300x64"] = prompt_scores_row(0, 300, 64, 4, 192)
ROWS["group_argmax"] = group_argmax_row
ROWS["retrieval_rank-null"] = retrieval_row("null")
ROWS["retrieval_rank-explicit"] = retrieval_row("explicit")
ROWS["refine-overlap"] = refine_row(True)
ROWS["refine-no_overlap"] = refine_row(False)
ROWS["resize_crop_uint8"] = resize_crop_row
ROWS["region_patches-256"] = region_patches_row
ROWS["score_reference-4097"] = sort_row(4097)
ROWS["score_reference-70001"] = sort_row(70001)
ROWS["boot_roc-global_slabs"] = boot_roc_row("slabs")
ROWS["boot_roc-300"] = boot_roc_row("lds")
ROWS["boot_confusion-2"] = boot_confusion_row(2)
ROWS["boot_confusion-7"] = boot_confusion_row(7)
ROWS["eval_roc-curve"] = eval_roc_row(True)
ROWS["eval_roc-scalars"] = eval_roc_row(False)
ROWS["region_grid-rule"] = region_grid_row(TissueRule(sat_min=20, min_fraction=0.25))
ROWS["region_grid-every_cell"] = region_grid_row(None)
ROWS["region_grid_mask"] = region_grid_mask_row
ROWS["tissue_mask"] = tissue_mask_row
ROWS["regions_label-1"] = regions_label_row(1)
ROWS["regions_label-50"] = regions_label_row(50)
ROWS["regions_feret"] = region_shape_row
ROWS["outline_count_trace"] = outlines_row
ROWS["outline_draw"] = outline_draw_row
ROWS["poly_fill-union"] = poly_fill_row("union", False)
ROWS["poly_fill-evenodd-into"] = poly_fill_row("evenodd", True)
ROWS["mask_dist2-foreground"] = mask_dist2_row("foreground")
ROWS["mask_dist2-background"] = mask_dist2_row("background")
ROWS["raster_peaks"] = raster_peaks_row(False)
ROWS["raster_peaks-tissue"] = raster_peaks_row(True)
ROWS["region_quality"] = region_quality_row
ROWS["heat_smooth"] = smooth_row(False)
ROWS["heat_smooth-tissue"] = smooth_row(True)
ROWS["cluster_seed_step"] = cluster_seed_row
ROWS["probe_loss_grad"] = probe_row
ROWS["pca_moments"] = pca_row
ROWS["topk-3_segments"] = topk_row
ROWS["knn_vote"] = knn_vote_row


@pytest.mark.parametrize("name", list(ROWS))
def test_result_does_not_depend_on_stale_workspace_bytes(towers, name):
    m, call, check, cls_buf = ROWS[name](towers)
    poison(m, call, check, cls_buf)


def test_fill_reports_what_it_filled():
    lib = _lib.load()
    n = C.c_int64(-1)
    assert lib.keep_debug_fill_workspace(None, 0, C.byref(n), None) == _lib.KEEP_EINVAL
    m = fresh()
    assert lib.keep_debug_fill_workspace(m._handle, 0, None, _stream(m._device)) == _lib.KEEP_EINVAL
    assert workspace(m) == 0 and fill(m, 0xFFFFFFFF) == 0                # no arena yet: nothing to fill, still KEEP_OK
    x = dev(family("normal", 5000))
    m.score_reference(x)
    W = workspace(m)
    assert W > 0 and fill(m, 0x7FC00000) == W and workspace(m) == W      # nothing allocated, nothing freed
