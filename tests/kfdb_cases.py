"""Seeded KeyFrameDatabase cases for the restatement (kfdb_ref) and the library.

BowVectors are drawn directly: strictly ascending words, positive values normalised to L1 = 1.
Keyframes come in "places": the members of a place draw most of their words from a common pool, so
a query near a place has a clear winner group and other places fall below the 0.8 threshold.
Covisible lists mix same-place keyframes, other places, excluded ids and ids absent from the
database.  A case is a list of steps, applied in order to the restatement (kfdb_ref.run_steps) and
to the library:
    ("add", id, bow) ("add_batch", ids, bows) ("erase", id) ("clear",) ("cov", id, ids)
    ("loop", bow, connected_ids, minScore) ("reloc", bow) ("reloc_batch", bows)
with bow = (uint32 words, float64 values)."""
import numpy as np

from kfdb_ref import l1_score

VOCAB = dict(k=10, L=3)          # 1,000 words: sharing is dense
VOCAB_BIG = dict(k=10, L=4)      # 10,000 words: room for a 4096-word BowVector
ABSENT = 100000                  # ids from here on are never added


def n_words(vocab):
    return vocab["k"] ** vocab["L"]


def make_bow(rng, words):
    w = np.unique(np.asarray(words, np.uint32))
    v = rng.uniform(0.05, 1.0, len(w))
    return w, (v / v.sum() if len(w) else v)


def place_pool(rng, nw, blen):
    return rng.choice(nw, size=min(nw, max(blen + blen // 3, 2)), replace=False)


def member(rng, pool, nw, blen, common=0.85):
    """A keyframe of the place: ~`common` of its words from the pool, the rest from anywhere."""
    nc = min(len(pool), max(1, int(round(blen * common))))
    w = set(rng.choice(pool, size=nc, replace=False).tolist())
    while len(w) < blen:
        w.add(int(rng.integers(0, nw)))
    return make_bow(rng, sorted(w)[:blen] if len(w) > blen else sorted(w))


def near(rng, bow, pool, nw, keep=0.9):
    """A view of the same scene as `bow`: most of its words, a few others, new values."""
    w = bow[0]
    nk = max(1, int(round(len(w) * keep)))
    s = set(rng.choice(w, size=nk, replace=False).tolist())
    while len(s) < len(w):
        s.add(int(rng.choice(pool)) if rng.random() < 0.5 else int(rng.integers(0, nw)))
    return make_bow(rng, sorted(s))


def world(seed, nkf, blen, vocab=VOCAB, nplaces=None, cov=True):
    """`nkf` keyframes (ids 0, 3, 6, ... in add order) in places, with their covisible lists."""
    rng = np.random.default_rng(seed)
    nw = n_words(vocab)
    nplaces = nplaces or max(1, min(6, nkf // 8))
    pools = [place_pool(rng, nw, blen) for _ in range(nplaces)]
    ids = [3 * i for i in range(nkf)]
    place = [int(rng.integers(0, nplaces)) for _ in ids]
    bows = [member(rng, pools[p], nw, blen) for p in place]
    covs = {}
    if cov:
        for i, kid in enumerate(ids):
            same = [ids[j] for j in range(nkf) if place[j] == place[i] and j != i]
            other = [ids[j] for j in range(nkf) if place[j] != place[i]]
            lst = []
            if same:
                lst += rng.choice(same, size=min(len(same), int(rng.integers(0, 7))), replace=False).tolist()
            if other:
                lst += rng.choice(other, size=min(len(other), int(rng.integers(0, 3))), replace=False).tolist()
            if rng.random() < 0.4:
                lst.append(ABSENT + int(rng.integers(0, 50)))
            rng.shuffle(lst)
            covs[kid] = [int(x) for x in lst[:10]]
    return dict(rng=rng, nw=nw, pools=pools, ids=ids, place=place, bows=bows, covs=covs, vocab=vocab)


def load_steps(W, batch=True):
    steps = [("cov", k, c) for k, c in W["covs"].items()]
    if batch:
        steps.append(("add_batch", list(W["ids"]), list(W["bows"])))
    else:
        steps += [("add", k, b) for k, b in zip(W["ids"], W["bows"])]
    return steps


def reloc_step(W, anchor):
    """A frame at the place of keyframe index `anchor`: a new view, as close to every member."""
    blen = len(W["bows"][anchor][0])
    return ("reloc", member(W["rng"], W["pools"][W["place"][anchor]], W["nw"], blen))


def loop_step(W, anchor, exclude_anchor=True, n_connected=3):
    """A new keyframe near keyframe index `anchor`.  Its connected set is the anchor (which would
    score best) and a few of the anchor's place-mates; minScore is the lowest score of the query
    against its connected keyframes, as LoopClosing::DetectLoop computes it (LoopClosing.cc:107-123)."""
    rng = W["rng"]
    q = near(rng, W["bows"][anchor], W["pools"][W["place"][anchor]], W["nw"])
    mates = [j for j in range(len(W["ids"])) if W["place"][j] == W["place"][anchor] and j != anchor]
    con = ([anchor] if exclude_anchor else []) + (
        rng.choice(mates, size=min(len(mates), n_connected), replace=False).tolist() if mates else [])
    ql = (q[0].tolist(), q[1].tolist())
    scores = [l1_score(ql, (W["bows"][j][0].tolist(), W["bows"][j][1].tolist())) for j in con]
    minScore = float(np.float32(min(scores))) if scores else 0.0
    connected = [W["ids"][j] for j in con] + [ABSENT + 77]
    return ("loop", q, connected, minScore)


def normal_case(name, seed, nkf, blen, vocab=VOCAB, exclude_anchor=True, batch=True):
    W = world(seed, nkf, blen, vocab)
    rng = W["rng"]
    steps = load_steps(W, batch)
    a1, a2 = int(rng.integers(0, nkf)), int(rng.integers(0, nkf))
    steps.append(reloc_step(W, a1))
    steps.append(loop_step(W, a2, exclude_anchor and nkf > 1))
    return dict(name=name, kind="normal", vocab=vocab, steps=steps)


def normal_cases():
    """Database sizes 1, 63, 64, 65, 300; BowVector lengths 1, 63, 64, 65, ~300, 4096."""
    C = [normal_case("kf1_len64", 11, 1, 64),
         normal_case("kf63_len65", 12, 63, 65),
         normal_case("kf64_len63", 13, 64, 63),
         normal_case("kf65_len64", 14, 65, 64),
         normal_case("kf300_len300", 15, 300, 300),
         normal_case("kf40_len1", 16, 40, 1),
         normal_case("kf40_len300_single_adds", 17, 40, 300, batch=False),
         normal_case("kf24_len120", 18, 24, 120),
         normal_case("kf48_len200", 19, 48, 200)]
    # one keyframe and one query at 4096 words among ordinary ones
    W = world(20, 9, 300, VOCAB_BIG, nplaces=1)
    rng = W["rng"]
    big = make_bow(rng, rng.choice(W["nw"], size=4096, replace=False))
    steps = load_steps(W) + [("add", 999, big), ("cov", 999, [0, 3]),
                             ("reloc", near(rng, big, W["pools"][0], W["nw"], keep=0.95)),
                             ("loop", near(rng, big, W["pools"][0], W["nw"], keep=0.95), [ABSENT], 0.01)]
    C.append(dict(name="kf10_len4096", kind="normal", vocab=VOCAB_BIG, steps=steps))
    return C


def lifecycle_case(seed=31):
    """erase of the first, a middle and the last keyframe; erase and re-add of one id (it moves to the
    end of the order); an absent erase; covisibles replaced between two queries; clear, then reuse."""
    W = world(seed, 30, 150, nplaces=2)
    rng = W["rng"]
    ids = W["ids"]
    steps = load_steps(W, batch=False)
    steps.append(reloc_step(W, 4))
    steps += [("erase", ids[0]), ("erase", ids[14]), ("erase", ids[-1]), ("erase", ABSENT + 5)]
    steps.append(reloc_step(W, 4))
    steps.append(loop_step(W, 7))
    steps += [("erase", ids[5]), ("add", ids[5], W["bows"][5])]           # same id, new sequence number
    steps.append(reloc_step(W, 5))
    steps.append(loop_step(W, 9))
    steps.append(("cov", ids[4], [ids[5], ids[6], ABSENT + 1, ids[7]]))
    steps.append(("cov", ids[6], []))
    steps.append(reloc_step(W, 4))
    steps.append(("clear",))
    steps.append(reloc_step(W, 4))                                          # empty database
    steps += [("add", ids[j], W["bows"][j]) for j in (9, 3, 12, 4, 5)]
    steps.append(reloc_step(W, 4))
    return dict(name="lifecycle", kind="lifecycle", vocab=VOCAB, steps=steps)


def batch_case(seed=41):
    """Relocalization batches of 1, 2 and 7 queries of unequal length, one with an empty query."""
    W = world(seed, 70, 130, nplaces=4)
    rng = W["rng"]
    nw = W["nw"]

    def q(a, blen=None):
        b = (near(rng, W["bows"][a], W["pools"][W["place"][a]], nw) if a % 2 else
             member(rng, W["pools"][W["place"][a]], nw, 130))
        return b if blen is None else (b[0][:blen], b[1][:blen])

    empty = (np.zeros(0, np.uint32), np.zeros(0))
    steps = load_steps(W)
    steps.append(("reloc_batch", [q(3)]))
    steps.append(("reloc_batch", [q(10), q(20, 40)]))
    steps.append(("reloc_batch", [q(1), q(2, 1), q(30, 64), q(31, 65), q(40), q(50, 63), q(60)]))
    steps.append(("reloc_batch", [q(5), empty, q(6)]))
    return dict(name="batch", kind="batch", vocab=VOCAB, steps=steps)


def _bow(words, values):
    return np.asarray(words, np.uint32), np.asarray(values, np.float64)


def boundary_cases():
    """Built by hand; values are dyadic so that every score is exact in float."""
    C = []
    # a keyframe with exactly minCommonWords shared words is not scored: max 10 -> min 8
    q10 = _bow(range(10), [0.1] * 10)
    steps = [("add", 1, _bow(range(10), [0.1] * 10)), ("add", 2, _bow(range(8), [0.125] * 8)),
             ("add", 3, _bow(range(1, 10), [1 / 9] * 9)), ("reloc", q10), ("loop", q10, [], 0.0)]
    C.append(dict(name="words_eq_minCommonWords", kind="boundary", vocab=VOCAB, steps=steps))
    # si == minScore is kept: query == keyframe 1 scores exactly 1; keyframe 2 scores exactly 0.75
    q = _bow([5, 6], [0.5, 0.5])
    steps = [("add", 1, _bow([5, 6], [0.5, 0.5])), ("add", 2, _bow([5, 6], [0.25, 0.75])),
             ("loop", q, [], 1.0), ("loop", q, [], 0.75), ("loop", q, [], 0.5)]
    C.append(dict(name="si_eq_minScore", kind="boundary", vocab=VOCAB, steps=steps))
    # accScore == 0.75f * bestAccScore is dropped: keyframe 1 scores 1, keyframe 2 scores 0.75
    q = _bow([5, 6, 7, 8], [0.25] * 4)
    steps = [("add", 1, _bow([5, 6, 7, 8], [0.25] * 4)), ("add", 2, _bow([5, 6, 7, 8], [0.5, 0.25, 0.125, 0.125])),
             ("add", 3, _bow([5, 6, 7, 8], [0.4375, 0.25, 0.1875, 0.125])), ("reloc", q), ("loop", q, [], 0.0)]
    C.append(dict(name="acc_eq_retain", kind="boundary", vocab=VOCAB, steps=steps))
    # two neighbours with equal scores above the entry's: the first stays best
    q = _bow([5, 6], [0.5, 0.5])
    steps = [("add", 1, _bow([5, 6], [0.125, 0.875])), ("add", 2, _bow([5, 6], [0.25, 0.75])),
             ("add", 3, _bow([5, 6], [0.75, 0.25])), ("cov", 1, [3, 2]), ("reloc", q), ("loop", q, [], 0.0),
             ("cov", 1, [2, 3]), ("reloc", q)]
    C.append(dict(name="equal_neighbours", kind="boundary", vocab=VOCAB, steps=steps))
    return C


def gpu_cases():
    """Every case the GPU tests compare with the restatement."""
    return normal_cases() + boundary_cases() + [lifecycle_case(), batch_case()]
