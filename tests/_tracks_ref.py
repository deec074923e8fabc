"""A plain restatement of tracks::TracksBuilder (Build / Filter / ExportToSTL, tracks/tracks.hpp:62-197, union_find.hpp) - the
expectation of the tests of mvgx_tracks_build - and the seeded match graphs the fixture generator and the tests share.
All outputs are integers: every comparison with this file is for equality."""
import numpy as np

SEED = 0x7AC5
N_FIXTURE = 160


class Result:
    def __init__(self, track_id, track_start, obs_image, obs_feature, counts):
        self.track_id, self.track_start, self.obs_image, self.obs_feature = track_id, track_start, obs_image, obs_feature
        self.counts = counts   # n_matches_used, n_nodes, n_components, n_collision, n_short, n_tracks, n_obs
        self.first_node = None  # per track: the smallest node index of its component (what a min-label implementation would report)


COUNTS = ("n_matches_used", "n_nodes", "n_components", "n_collision", "n_short", "n_tracks", "n_obs")


def compacted(pairs, match_start, ij, match_mask):
    """the lists with the masked matches removed (what the reference would be handed)"""
    pairs = np.asarray(pairs, np.uint32).reshape(-1, 2)
    start = np.asarray(match_start, np.int64).reshape(-1)
    ij = np.asarray(ij, np.uint32).reshape(-1, 2)
    keep = np.asarray(match_mask, bool).reshape(-1)[: len(ij)]
    kept_before = np.concatenate([[0], np.cumsum(keep)])
    return pairs, kept_before[start].astype(np.uint64) if len(start) else np.zeros(1, np.uint64), ij[keep]


def build(pairs, match_start, ij, match_mask=None, min_length=2):
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    start = np.asarray(match_start, np.int64).reshape(-1)
    ij = np.asarray(ij, np.int64).reshape(-1, 2)
    n_pairs = len(pairs)
    # the matches in container order, the mask applied
    rows = []
    for p in range(n_pairs):
        lo, hi = int(start[p]), int(start[p + 1])
        m = ij[lo:hi]
        if match_mask is not None:
            m = m[np.asarray(match_mask[lo:hi], bool)]
        rows.append(np.stack([np.full(len(m), pairs[p, 0]), m[:, 0], np.full(len(m), pairs[p, 1]), m[:, 1]], axis=1))
    m = np.concatenate(rows) if rows else np.zeros((0, 4), np.int64)
    # Build: node = rank of (image, feature) among the distinct ones (:74-100)
    key = np.concatenate([m[:, 0] << 32 | m[:, 1], m[:, 2] << 32 | m[:, 3]])
    nodes = np.unique(key)
    a = np.searchsorted(nodes, m[:, 0] << 32 | m[:, 1])
    b = np.searchsorted(nodes, m[:, 2] << 32 | m[:, 3])
    n = len(nodes)
    parent, rank = list(range(n)), [0] * n

    def find(i):
        r = i
        while parent[r] != r:
            r = parent[r]
        while parent[i] != r:   # path compression (:63-72); it changes neither a rank nor a root
            parent[i], i = r, parent[i]
        return r

    for x, y in zip(a.tolist(), b.tolist()):   # Union (:75-103), one per match in order
        i, j = find(x), find(y)
        if i == j:
            continue
        if rank[i] < rank[j]:
            parent[i] = j
        else:
            parent[j] = i
            if rank[i] == rank[j]:
                rank[i] += 1
    root = np.array([find(k) for k in range(n)], np.int64)
    image, feature = nodes >> 32, nodes & 0xFFFFFFFF
    # Filter (:124-165)
    order = np.lexsort((np.arange(n), root))   # by track id, then node = ascending (image, feature)
    r_s, im_s = root[order], image[order]
    ids, first, size = np.unique(r_s, return_index=True, return_counts=True)
    twice = np.zeros(len(ids), bool)
    same = (r_s[1:] == r_s[:-1]) & (im_s[1:] == im_s[:-1])   # nodes of a track ascend in (image, feature): a repeated image is adjacent
    twice[np.searchsorted(ids, r_s[1:][same])] = True
    short = ~twice & (size < min_length)
    keep = ~twice & ~short
    # ExportToSTL (:178-196): ascending track id, ascending image inside
    sel = np.repeat(keep, size)
    res = Result(ids[keep].astype(np.uint32), np.concatenate([[0], np.cumsum(size[keep])]).astype(np.uint64), im_s[sel].astype(np.uint32),
                 feature[order][sel].astype(np.uint32),
                 dict(n_matches_used=len(m), n_nodes=n, n_components=len(ids), n_collision=int(twice.sum()), n_short=int(short.sum()),
                      n_tracks=int(keep.sum()), n_obs=int(size[keep].sum())))
    res.first_node = order[first][keep].astype(np.uint32)
    return res


# ---- seeded match graphs ----
def container(lists):
    """{(I, J): [(i, j), ...]} -> pairs, match_start, ij in the order of a std::map<Pair, IndMatches>"""
    keys = sorted(lists)
    pairs = np.array(keys, np.uint32).reshape(-1, 2)
    start = np.concatenate([[0], np.cumsum([len(lists[k]) for k in keys])]).astype(np.uint64)
    ij = np.array([m for k in keys for m in lists[k]], np.uint32).reshape(-1, 2)
    return pairs, start, ij


def random_graph(rng, n_images, n_points, wrong=0.08, duplicates=0.05, missing=0.2, visible=0.6, spread=None):
    """Points seen in random subsets of the images, every image numbering its features in a random order; every pair of images is
    matched on the points both see, except the `missing` share of the pairs; a `wrong` share of the matches is redirected to another
    feature of J, a `duplicates` share is repeated inside its list, every list is shuffled. spread: feature indices are mapped into
    [0, spread) (sparse indices). Returns (n_images, pairs, match_start, ij, features per image)."""
    sees = rng.random((n_images, n_points)) < visible
    feat = np.full((n_images, n_points), -1, np.int64)
    count = np.zeros(n_images, np.int64)
    for I in range(n_images):
        pts = np.flatnonzero(sees[I])
        count[I] = len(pts) + int(rng.integers(0, 3))   # a few features no match uses
        ids = rng.permutation(count[I])[: len(pts)]
        if spread:
            ids = np.sort(rng.choice(spread, size=count[I], replace=False))[ids]
            count[I] = spread
        feat[I, pts] = ids
    lists = {}
    for I in range(n_images):
        for J in range(I + 1, n_images):
            if rng.random() < missing:
                continue
            both = np.flatnonzero(sees[I] & sees[J])
            ms = []
            for p in both:
                j = feat[J, p]
                if rng.random() < wrong:
                    j = feat[J, rng.choice(np.flatnonzero(sees[J]))]
                ms.append((int(feat[I, p]), int(j)))
                if rng.random() < duplicates:
                    ms.append(ms[int(rng.integers(0, len(ms)))])
            ms = [ms[k] for k in rng.permutation(len(ms))]
            lists[(I, J)] = ms
    pairs, start, ij = container(lists)
    return n_images, pairs, start, ij, count.astype(np.uint32)


def fixture_cases():
    """the cases of tests/golden/tracks_golden.npz: graphs of 2-8 images and 3-40 points; every fourth with n_features given, every
    twentieth with sparse feature indices up to 70 000 and n_features left out, every fifth with one more image that no pair names"""
    out = []
    for c in range(N_FIXTURE):
        rng = np.random.default_rng([SEED, c])
        sparse = c % 20 == 5
        n_images, pairs, start, ij, count = random_graph(rng, int(rng.integers(2, 9)), int(rng.integers(3, 41)), spread=70000 if sparse else None)
        if c % 5 == 2:
            n_images += 1
            count = np.concatenate([count, [4]]).astype(np.uint32)
        out.append(dict(name=f"fixture-{c}", n_images=n_images, n_features=count if (c % 4 == 1 and not sparse) else None, pairs=pairs, match_start=start, ij=ij))
    return out


def large_graph(seed, n_images=40, n_points=9000, visible=0.12):
    """about 10^5 matches"""
    rng = np.random.default_rng([SEED, 1000 + seed])
    n_images, pairs, start, ij, count = random_graph(rng, n_images, n_points, wrong=0.05, duplicates=0.01, missing=0.1, visible=visible)
    return dict(name=f"large-{seed}", n_images=n_images, n_features=count, pairs=pairs, match_start=start, ij=ij)
