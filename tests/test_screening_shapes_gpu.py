"""Prompt screening, group argmax, retrieval rank and keep_classify's second look, off the shapes of the golden files.

1. ``keep_prompt_scores`` in its three modes (``fused_screening`` = 0 unfused fp32, 1 fused MX-fp4-compensated, 2 fused three-pass) over
   more than one 256-column tile, ragged column tiles, row counts around the 256-row tile and its 128-row wave halves, C = 2 .. 5 and
   D = 640 / 192, against the float64 restatement of ``rank_cls_score``.
2. The loops over 256 MiB logit chunks of ``keep_prompt_scores`` (unfused), ``keep_group_argmax`` and ``keep_retrieval_rank``, crossed with
   wide, shallow problems at D = 32, plus the small shapes of ``keep_group_argmax`` (C = 1, 3, 5; N = 1, 5).
3. ``keep_classify``: flag / compact / gather / strict re-encode in sub-batches / scatter, row by row.

References are float64 on the host, computed in row blocks from the float32 inputs the engine gets.  The one exception is part 3: there
the code under test is the plumbing around the encoder, so the flagged rows are compared with the engine's own ``strict`` features (that
mode is pinned to the oracle in tests/test_towers_gpu.py).

Before a score vector is compared, guards are asserted on the REFERENCE alone: shifting it by one classifier, shifting it by 64
classifiers (one column tile at C = 4) and leaving out the last tile rows each move most entries by more than 2e-4 = 100 x the tolerance,
so a mis-indexed, shifted or truncated result cannot pass.
"""
import numpy as np
import pytest
import torch

import mx_reference as R
from keep_amd import KEEPModel, _lib
from keep_amd.config import small_shape
from keep_amd.model import _ptr, _stream
from keep_amd.synth import synth_state_dict, towers_of

pytestmark = pytest.mark.gpu

SCORE_TOL = 2e-6          # per score: the bound tests/test_wsi_gpu.py holds at the golden shape
GUARD_MOVE = 2e-4         # 100 x SCORE_TOL
# fused_screening = 1 takes its logits from the MX-fp4-compensated product A_hi W_hi^T + Q4(A_hi) Q4(W_lo)^T + Q4(A_lo) Q4(W_hi)^T, which is
# 1.9e-6 rms (up to 1e-5) away from the exact logit on these inputs.  The means over tiles keep that error where the tiles resemble each
# other, as they do here (cosine ~0.4 between any two): measured on the MI355X against float64, and equal to three digits to what the
# host emulation of the format (tests/mx_reference.py) gives for the same inputs,
#   N = 517: 4.11e-6   130 (C = 2): 4.29e-6   1: 9.83e-6   129: 2.78e-6   256: 3.26e-6   257: 2.74e-6   300 (D = 640): 2.80e-6
# while modes 0 and 2 stay below 6e-7 on every case.  So mode 1 is held to twice the largest of these against float64 -- the sums run in
# a fixed order, the factor is for other seeds only -- and to SCORE_TOL against the emulated product, which is the arithmetic it is meant
# to carry out.  (On the golden slide, whose tiles are not clustered, mode 1 is within 2e-6 of float64: tests/test_wsi_gpu.py.)
MODE1_TOL = 2 * 9.83e-6


# ------------------------------------------------------------------ inputs and float64 references
def screening_inputs(N, K, C, D, seed):
    """Features clustered round one centre, bank rows pulled towards +/- that centre by a per-row amount: cosines up to ~0.5 and scores
    that differ widely between classifiers (bare N(0,1) vectors give every classifier nearly the same score)."""
    g = torch.Generator().manual_seed(seed)
    centre = torch.rand(D, generator=g)
    feats = torch.nn.functional.normalize(torch.randn(N, D, generator=g) + 1.5 * centre, dim=-1)
    u = torch.rand(K * C, 1, generator=g) * 2 - 1
    bank = torch.nn.functional.normalize(torch.randn(K * C, D, generator=g) + 1.5 * centre * u, dim=-1)
    return feats, bank


def score_sums(feats, bank, K, C, r0, r1, block=1024):
    """float64 sum over tile rows [r0, r1) of (v1 - v2) - |v1 + v2 - 1| per classifier; v1, v2 the two largest of its C logits."""
    bt = bank.double().t()
    total = torch.zeros(K, dtype=torch.float64)
    for a in range(r0, r1, block):
        logits = (feats[a:min(a + block, r1)].double() @ bt).view(-1, K, C)
        v = logits.topk(2, dim=2).values
        total += ((v[..., 0] - v[..., 1]) - (v[..., 0] + v[..., 1] - 1).abs()).sum(0)
    return total


def reference_scores(feats, bank, K, C, drops=()):
    """float64 numpy scores over all N rows, and for each d of `drops` the scores with the last d rows left out."""
    N = feats.shape[0]
    cuts = sorted({N - d for d in drops if 0 < d < N}) + [N]
    sums, acc, lo = {}, torch.zeros(K, dtype=torch.float64), 0
    for hi in cuts:
        acc = acc + score_sums(feats, bank, K, C, lo, hi)
        sums[hi], lo = acc, hi
    return (sums[N] / N).numpy(), {d: (sums[N - d] / (N - d)).numpy() for d in drops if 0 < d < N}


def moved(a, b, by=GUARD_MOVE):
    return float((np.abs(a - b) > by).mean())


def assert_roll_guards(ref, K):
    """On the reference alone.  A roll that misses 90 % -> change the seed, not the guard."""
    assert moved(ref, np.roll(ref, 1)) > 0.9
    if K > 64:
        assert moved(ref, np.roll(ref, 64)) > 0.9


def fused(C, D):
    """Whether keep_prompt_scores takes the fused GEMM for this shape when fused_screening is 1 or 2."""
    return C in (2, 4) and D % 128 == 0 and D >= 256


def emulated_mode1_scores(feats, bank, K, C):
    """float64 scores from the float64 value of the compensated product (mx_reference.emulate, two correction terms)."""
    logits = torch.from_numpy(np.asarray(R.emulate(feats.numpy(), bank.numpy(), terms=2), dtype=np.float64)).view(-1, K, C)
    v = logits.topk(2, dim=2).values
    return (((v[..., 0] - v[..., 1]) - (v[..., 0] + v[..., 1] - 1).abs()).sum(0) / logits.shape[0]).numpy()


def engine_scores(m, feats_d, bank_d, K, C):
    N, D = feats_d.shape
    out = torch.empty(K, dtype=torch.float32, device=feats_d.device)
    rc = _lib.load().keep_prompt_scores(m._handle, _ptr(feats_d), _ptr(bank_d), N, K, C, D, _ptr(out), _stream(feats_d.device))
    _lib.check(m._handle, rc, "prompt_scores")
    return out.cpu().double().numpy()


@pytest.fixture(scope="module")
def engines():
    """One weight-less handle per screening mode (the option cannot be read back, so it is never changed on a shared handle)."""
    out = {}
    for mode in (0, 1, 2):
        m = KEEPModel()
        m.set_option("fused_screening", mode)
        m._ready_device()
        out[mode] = m
    return out


# ------------------------------------------------------------------ 1. column tiles, row tails, C, D
# Truncation guard.  Leaving out ONE row moves a score by |row score - mean| / (N - 1).  With this recipe a row's score deviates from
# the mean by about 0.05 (the noise part of a feature projects onto a bank row with sigma = 768^-1/2), so one row moves more than 2e-4
# in 57-59 % of the classifiers at N = 129 / 130, 23-50 % at N = 256 .. 300 and 3 % at N = 517 (measured on the host): the 90 % of the
# two roll guards is out of reach for one row.  Chosen instead, both asserted for every case with N > 1:
#   * the last max(1, N // 8) rows left out move more than TRUNC_SHARE = 70 % of the entries by more than 2e-4 (host: 80-97 %);
#   * the last ONE row left out moves more than 70 % of the entries by more than 2e-5 = 10 x the tolerance (host: 78-96 %).
TRUNC_SHARE = 0.7
SCREEN_CASES = [
    (517, 449, 4, 768),      # 1 796 columns: 8 column tiles, ragged last one, two reduce workgroups
    (130, 901, 2, 768),      # C = 2: two scores per lane; K above 3 x 256
    (1, 65, 4, 768),         # one row (nothing to truncate); crosses one column tile
    (129, 65, 4, 768),       # the second wm half of the workgroup holds one valid row
    (256, 64, 4, 768),       # exactly one full tile, no padding in either direction
    (257, 64, 4, 768),       # one full tile plus one row
    (300, 200, 3, 768),      # C = 3: always unfused
    (300, 200, 5, 768),      # C = 5: always unfused
    (300, 64, 4, 640),       # D a multiple of 128 other than 768
    (300, 64, 4, 192),       # D below 256: unfused
]
_screen_cache = {}


def screening_case(N, K, C, D):
    key = (N, K, C, D)
    if key not in _screen_cache:
        feats, bank = screening_inputs(N, K, C, D, seed=N * 7 + K * 3 + C + D)
        ref, trunc = reference_scores(feats, bank, K, C, drops=(1, max(1, N // 8)))
        _screen_cache[key] = {"feats": feats, "bank": bank, "ref": ref, "trunc": trunc}
    return _screen_cache[key]


def assert_screening_guards(case, N, K):
    ref, trunc = case["ref"], case["trunc"]
    assert_roll_guards(ref, K)
    if N > 1:
        assert moved(ref, trunc[max(1, N // 8)]) > TRUNC_SHARE
        assert moved(ref, trunc[1], by=10 * SCORE_TOL) > TRUNC_SHARE


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("N,K,C,D", SCREEN_CASES)
def test_prompt_scores_over_column_tiles_row_tails_and_C(engines, N, K, C, D, mode):
    case = screening_case(N, K, C, D)
    ref = case["ref"]
    assert_screening_guards(case, N, K)
    if "feats_d" not in case:
        case["feats_d"], case["bank_d"] = case["feats"].cuda(), case["bank"].cuda()
    got = engine_scores(engines[mode], case["feats_d"], case["bank_d"], K, C)
    err = float(np.abs(got - ref).max())
    print(f"[prompt_scores N={N} K={K} C={C} D={D} fused_screening={mode}] max err vs float64 {err:.2e}; score spread {ref.max() - ref.min():.2f}")
    assert got.shape == (K,)
    if mode == 1 and fused(C, D):
        if "emulated" not in case:
            case["emulated"] = emulated_mode1_scores(case["feats"], case["bank"], K, C)
        err_model = float(np.abs(got - case["emulated"]).max())
        print(f"    vs the emulated MX-fp4-compensated product {err_model:.2e}; the emulation itself vs float64 {np.abs(case['emulated'] - ref).max():.2e}")
        assert err < MODE1_TOL and err_model < SCORE_TOL
    else:
        assert err < SCORE_TOL


# ------------------------------------------------------------------ 2. more than one logit chunk
WIDE_N, WIDE_K, WIDE_C, WIDE_D = 8500, 2000, 4, 32          # 8 000 columns -> chunks of 2^26 / 8 000 = 8 388 rows: 8 388 + 112
WIDE_CHUNK = (1 << 26) // (WIDE_K * WIDE_C)
WIDE_TIED = (3, 1000, 1999)                                 # classifiers whose class rows 1 and 3 are identical


@pytest.fixture(scope="module")
def wide():
    """Inputs and float64 references shared by the two multi-chunk tests; built once and not written afterwards."""
    assert WIDE_CHUNK == 8388 and WIDE_CHUNK < WIDE_N
    N, K, C, D = WIDE_N, WIDE_K, WIDE_C, WIDE_D
    feats, bank = screening_inputs(N, K, C, D, seed=2026)
    for k in WIDE_TIED:
        bank[k * C + 3] = bank[k * C + 1]
    bt = bank.double().t()
    sums = torch.zeros(2, K, dtype=torch.float64)            # per chunk
    exp = torch.empty(N, K, dtype=torch.int8)
    clear = torch.empty(N, K, dtype=torch.bool)
    tied = torch.zeros(N, K, dtype=torch.bool)
    for a in range(0, N, 1024):
        b = min(a + 1024, N)
        logits = (feats[a:b].double() @ bt).view(-1, K, C)
        v = logits.topk(2, dim=2).values
        s = (v[..., 0] - v[..., 1]) - (v[..., 0] + v[..., 1] - 1).abs()
        in0 = torch.arange(a, b) < WIDE_CHUNK                # a block may straddle the chunk boundary
        sums[0] += s[in0].sum(0)
        sums[1] += s[~in0].sum(0)
        exp[a:b] = logits.argmax(2).to(torch.int8)           # first maximum wins
        # the gap that decides a label: with the copy of class 1 (class 3 of the tied classifiers) left out
        dec = logits.clone()
        for k in WIDE_TIED:
            dec[:, k, 3] = -np.inf
        w = dec.topk(2, dim=2).values
        clear[a:b] = (w[..., 0] - w[..., 1]) > 1e-6
        for k in WIDE_TIED:
            tied[a:b, k] = clear[a:b, k] & (exp[a:b, k] == 1)
    return {"feats": feats, "bank": bank, "feats_d": feats.cuda(), "bank_d": bank.cuda(),
            "scores": ((sums[0] + sums[1]) / N).numpy(), "scores_one_chunk": [(sums[0] / N).numpy(), (sums[1] / N).numpy()],
            "exp": exp, "clear": clear, "tied": tied}


def test_prompt_scores_across_two_logit_chunks(engines, wide):
    """D = 32 puts every mode on the unfused path; `sums` must accumulate over both chunks.  One row of 8 500 moves a score by far less
    than the guard, so the truncation guard here is the one this loop can get wrong: what the engine would return had it kept the sum of
    one chunk only (first or second), still divided by N."""
    ref = wide["scores"]
    assert_roll_guards(ref, WIDE_K)
    for one in wide["scores_one_chunk"]:
        assert moved(ref, one) > 0.9
    for mode in (0, 1, 2):
        got = engine_scores(engines[mode], wide["feats_d"], wide["bank_d"], WIDE_K, WIDE_C)
        err = float(np.abs(got - ref).max())
        print(f"[prompt_scores two chunks, fused_screening={mode}] max err vs float64 {err:.2e}; score spread {ref.max() - ref.min():.2f}")
        assert err < SCORE_TOL


def engine_group_argmax(m, feats_d, bank_d, K, C):
    N, D = feats_d.shape
    out = torch.full((N, K), -1, dtype=torch.int32, device=feats_d.device)
    rc = _lib.load().keep_group_argmax(m._handle, _ptr(feats_d), _ptr(bank_d), N, K, C, D, _ptr(out), _stream(feats_d.device))
    _lib.check(m._handle, rc, "group_argmax")
    return out.cpu()


def test_group_argmax_across_two_logit_chunks(engines, wide):
    exp, clear, tied = wide["exp"], wide["clear"], wide["tied"]
    left_out = int((~clear).sum())
    assert left_out < 0.01 * clear.numel()
    for rows in (slice(0, WIDE_CHUNK), slice(WIDE_CHUNK, WIDE_N)):       # ties decided by the rule in BOTH chunks
        assert int(tied[rows].sum()) >= 3
    got = engine_group_argmax(engines[0], wide["feats_d"], wide["bank_d"], WIDE_K, WIDE_C)
    print(f"[group_argmax two chunks] {left_out} of {clear.numel()} entries left out (float64 top-2 gap <= 1e-6); {int(tied.sum())} entries decided by the tie rule")
    assert int(got.min()) >= 0 and int(got.max()) < WIDE_C
    for rows in (slice(0, WIDE_CHUNK), slice(WIDE_CHUNK, WIDE_N)):
        g, e, c = got[rows], exp[rows].to(torch.int32), clear[rows]
        assert torch.equal(g[c], e[c])
        assert (g[tied[rows]] == 1).all()
    for k in WIDE_TIED:
        assert not (got[:, k] == 3).any()                    # the copy at the higher index never wins


@pytest.mark.parametrize("C", [1, 3, 5])
@pytest.mark.parametrize("N", [1, 5])
def test_group_argmax_small_shapes(engines, N, C):
    K, D = 50, 768
    g = torch.Generator().manual_seed(100 * N + C)
    feats = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=-1)
    bank = torch.nn.functional.normalize(torch.randn(K * C, D, generator=g), dim=-1)
    logits = (feats.double() @ bank.double().t()).view(N, K, C)
    exp = logits.argmax(2).to(torch.int32)
    got = engine_group_argmax(engines[0], feats.cuda(), bank.cuda(), K, C)
    if C == 1:
        assert int(got.abs().sum()) == 0
        return
    top2 = logits.topk(2, dim=2).values
    clear = (top2[..., 0] - top2[..., 1]) > 1e-6
    assert int((~clear).sum()) < 0.01 * clear.numel()
    assert torch.equal(got[clear], exp[clear]) and int(got.min()) >= 0 and int(got.max()) < C


RET_N, RET_P, RET_D = 70000, 1000, 32                       # chunks of 2^26 / 70 000 = 958 captions: 958 + 42
RET_CHUNK = (1 << 26) // RET_N


def retrieval_reference(img, txt, target, block=100):
    """Position of image target[p] in caption p's descending similarity list: float64 scores, stable ascending sort read backwards
    (`arr.argsort()[-k:][::-1]` lists equal scores with the higher index first).  Also the rows where another image scores within 1e-6
    of the target without being equal to it: there the float32 engine may legitimately differ."""
    N = img.shape[0]
    it = img.double().t()
    rank = torch.empty(txt.shape[0], dtype=torch.int64)
    close = torch.empty(txt.shape[0], dtype=torch.bool)
    for a in range(0, txt.shape[0], block):
        s = txt[a:a + block].double() @ it
        order = torch.sort(s, dim=1, stable=True).indices
        t = target[a:a + block]
        pos = (order == t[:, None]).int().argmax(1)
        rank[a:a + block] = N - 1 - pos
        d = (s - s.gather(1, t[:, None])).abs()
        close[a:a + block] = ((d <= 1e-6) & (d > 0)).any(1)
    return rank, close


@pytest.fixture(scope="module")
def retrieval():
    assert RET_CHUNK == 958 and RET_CHUNK < RET_P
    g = torch.Generator().manual_seed(77)
    img = torch.nn.functional.normalize(torch.randn(RET_N, RET_D, generator=g), dim=-1)
    # exact duplicates at a HIGHER index of images that captions of both chunks look for: they count as "above" the target
    dups = {5: 60005, 400: 69999, 970: 31000, 985: 61234, 999: 1000}
    for src, dst in dups.items():
        img[dst] = img[src]
    own = torch.arange(RET_P)                                                      # target = null: caption p looks for image p
    other = (own * 67 + 12345) % RET_N                                             # explicit targets, none equal to its row index
    other[960], other[990] = 61234, 31000                                          # the copy is the target: the original below it does not count
    assert not (other == own).any() and other.unique().numel() == RET_P
    cases = {}
    for name, tgt in (("null", own), ("explicit", other)):
        # captions at cosine 0.45 .. 0.8 to their image: ranks from 0 to a few thousand, and few other images within 1e-6 of the target
        a = torch.rand(RET_P, 1, generator=g) * 1.2 + 0.8
        noise = torch.nn.functional.normalize(torch.randn(RET_P, RET_D, generator=g), dim=-1)
        txt = torch.nn.functional.normalize(img[tgt] + a * noise, dim=-1)
        rank, close = retrieval_reference(img, txt, tgt)
        cases[name] = {"txt": txt, "target": tgt, "rank": rank, "close": close}
    return {"img": img, "cases": cases, "dups": dups}


@pytest.mark.parametrize("targets", ["null", "explicit"])
def test_retrieval_rank_across_two_caption_chunks(engines, retrieval, targets):
    case = retrieval["cases"][targets]
    rank, close, tgt = case["rank"], case["close"], case["target"]
    assert int(close.sum()) <= 0.01 * RET_P
    second = torch.arange(RET_P) >= RET_CHUNK
    assert int((rank[second] > 0).sum()) > 10 and int(rank.max()) > 50             # the second chunk is not all zeros; ranks spread
    if targets == "null":
        for src in retrieval["dups"]:
            assert rank[src] >= 1                                                  # the copy at the higher index counts as above
    m = engines[0]
    if "img_d" not in retrieval:
        retrieval["img_d"] = retrieval["img"].cuda()
    img_d, txt_d = retrieval["img_d"], case["txt"].cuda()
    tgt_d = None if targets == "null" else tgt.to(torch.int32).cuda()
    out = torch.full((RET_P,), -1, dtype=torch.int32, device=img_d.device)
    rc = _lib.load().keep_retrieval_rank(m._handle, _ptr(txt_d), _ptr(img_d), RET_P, RET_N, RET_D, _ptr(tgt_d), _ptr(out), _stream(img_d.device))
    _lib.check(m._handle, rc, "retrieval_rank")
    got = out.cpu().long()
    print(f"[retrieval_rank two chunks, target {targets}] {int(close.sum())} of {RET_P} rows left out; largest rank {int(rank.max())}; "
          f"rows differing {int((got != rank)[~close].sum())}")
    assert torch.equal(got[~close], rank[~close])


# ------------------------------------------------------------------ 3. keep_classify's second look, row by row
def _model(sd, precision):
    m = KEEPModel(precision=precision, towers=towers_of(sd))
    m.load_state_dict(sd, strict=True)
    return m.to("cuda:0").eval()


def near_tie_bank():
    """The bank of test_near_tie_argmax: 8 prompts, each with a twin nudged by 3e-3 along one random direction, so top-2 margins spread
    over several decades."""
    g = torch.Generator().manual_seed(99)
    text_bank = torch.nn.functional.normalize(torch.randn(64, 768, generator=g), dim=-1)
    gen = torch.Generator().manual_seed(10)
    u = torch.nn.functional.normalize(torch.randn(768, generator=gen), dim=0)
    pairs = []
    for t1 in text_bank[:8]:
        pairs += [t1, torch.nn.functional.normalize(t1 + 3e-3 * u, dim=0)]
    return torch.stack(pairs)


def host_margins(sim):
    """float32, as top2_margin_flag_kernel takes them: v1 - v2 of each row."""
    top2 = sim.cpu().topk(2, dim=1).values
    return (top2[:, 0] - top2[:, 1]).numpy()


@pytest.fixture(scope="module")
def second_look_models():
    sd = synth_state_dict(small_shape(2, 2), seed=5, text=False)
    return _model(sd, "comp"), _model(sd, "strict")


@pytest.mark.parametrize("kind,B,want,anchors", [("f32", 1300, 300, (0, 1299, 1023, 1024)), ("u8", 300, 40, (0, 299))])
def test_classify_second_look_row_by_row(second_look_models, kind, B, want, anchors):
    """`want` flagged tiles: 300 of 1 300 is more than 256, hence two equal sub-batches, and the compaction carries its count across the
    1 024-wide iteration; tile 0, the last tile and both neighbours of index 1 024 are flagged.  Which tiles come out near a tie is a
    property of the random pixels, so a preliminary pass finds the tiles with the smallest margins and the batch is reordered to put
    them at those positions; everything below is measured on the reordered batch."""
    m, ms = second_look_models
    bank = near_tie_bank().cuda()
    g = torch.Generator(device="cuda").manual_seed(123)
    if kind == "f32":
        x = torch.randn(B, 3, 224, 224, device="cuda", generator=g)
    else:
        x = torch.randint(0, 256, (B, 224, 224, 3), dtype=torch.uint8, device="cuda", generator=g)
    s_pre, _ = m.classify(x, bank, margin=0.0)
    nearest = np.argsort(host_margins(s_pre), kind="stable")[:len(anchors)].tolist()
    perm = list(range(B))
    for a, c in zip(anchors, nearest):
        i = perm.index(c)
        perm[a], perm[i] = perm[i], perm[a]
    x = x[torch.tensor(perm, device="cuda")].contiguous()

    # 1. the first pass alone   2. the flag rule on the host, float32   3. a margin between two adjacent sorted margins
    s0, l0, f0 = m.classify(x, bank, margin=0.0, return_features=True)
    assert m.last_rechecked == 0
    d = host_margins(s0)
    srt = np.sort(d)
    i = want
    while not srt[i - 1] < np.float32((srt[i - 1] + srt[i]) / 2):          # (equal neighbours: move on to the next gap)
        i += 1
    margin = np.float32((srt[i - 1] + srt[i]) / 2)
    flagged = ~(d >= margin)                                             # !(v1 - v2 >= margin * scale), scale = 1
    count = int(flagged.sum())
    assert want <= count <= want + 20 and (count > 256) == (want > 256)
    assert all(flagged[a] for a in anchors)
    if B > 1024:
        assert flagged[:1024].any() and flagged[1024:].any()

    sim, lab, feats = m.classify(x, bank, margin=float(margin), return_features=True)
    assert m.last_rechecked == count
    fl = torch.from_numpy(flagged)
    sim, lab, feats, s0, f0 = sim.cpu(), lab.cpu(), feats.cpu(), s0.cpu(), f0.cpu()
    assert torch.equal(feats[~fl], f0[~fl]) and torch.equal(sim[~fl], s0[~fl])          # untouched rows: bit-identical
    strict = (ms.encode_image(x) if kind == "f32" else ms.encode_image_uint8(x)).cpu()
    e_feat = float((feats[fl] - strict[fl]).abs().max())
    e_sim = float((sim[fl].double() - feats[fl].double() @ bank.cpu().double().t()).abs().max())
    changed = float((feats[fl] != f0[fl]).any(1).float().mean())
    print(f"[second look {kind}] {count} of {B} tiles flagged at margin {float(margin):.3e}; flagged rows vs strict {e_feat:.2e}; "
          f"their sims vs features @ bank.T {e_sim:.2e}; {100 * changed:.0f} % of them differ from the first pass")
    assert changed >= 0.9                                                 # else a scattered row could not be told from an untouched one
    assert e_feat < 2e-6                                                  # the bound of test_classify_edge_cases
    assert e_sim < 1e-6
    assert torch.equal(lab.long(), sim.argmax(1))
