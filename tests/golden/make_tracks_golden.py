"""Writes tests/golden/tracks_golden.npz: the REFERENCE's tracks::TracksBuilder (Build, Filter(2) and Filter(3), ExportToSTL) on the
match graphs of tests/_tracks_ref.fixture_cases, next to the inputs.
Run by hand on the machine that has the reference tree (REFERENCE_SRC, default /root/reference/src): the small driver below - our own
text - is compiled against that tree into a temporary directory outside the repository, run once, and deleted; nothing compiled is kept.

The fixture is written only if the restatement (tests/_tracks_ref.py) equals the compiled reference on every case, and only if the cases
hold what the tests need: components with a repeated image, components dropped for their length at min_length 3 alone, and tracks whose
id is not their smallest node.

  python tests/golden/make_tracks_golden.py                 writes the fixture
  python tests/golden/make_tracks_golden.py --time DIR      times the compiled reference (Build + Filter(2) + ExportToSTL, one thread,
                                                            the median of five) on DIR/pairs.npy, match_start.npy, ij.npy - the files
                                                            tools/time_tracks.py writes - and prints one JSON line
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import _tracks_ref as tref  # noqa: E402

GOLD_PATH = os.path.join(ROOT, "tests", "golden", "tracks_golden.npz")
SRC = os.environ.get("REFERENCE_SRC", "/root/reference/src")

DRIVER = r"""
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <vector>
#include "openMVG/tracks/tracks.hpp"
using namespace openMVG;
static bool get(FILE* in, void* p, size_t bytes) { return fread(p, 1, bytes, in) == bytes; }
static void put(FILE* out, const void* p, size_t bytes) { fwrite(p, 1, bytes, out); }
static bool read_case(FILE* in, matching::PairWiseMatches& matches) {
  uint32_t n_pairs = 0;
  if (!get(in, &n_pairs, 4)) return false;
  for (uint32_t p = 0; p < n_pairs; ++p) {
    uint32_t head[3];   // I, J, length
    if (!get(in, head, 12)) return false;
    std::vector<uint32_t> ij(2 * (size_t)head[2]);
    if (head[2] && !get(in, ij.data(), 4 * ij.size())) return false;
    matching::IndMatches& list = matches[{head[0], head[1]}];
    for (uint32_t k = 0; k < head[2]; ++k) list.emplace_back(ij[2 * k], ij[2 * k + 1]);
  }
  return true;
}
static void run(const matching::PairWiseMatches& matches, uint32_t min_length, tracks::STLMAPTracks& out) {
  tracks::TracksBuilder builder;
  builder.Build(matches);
  builder.Filter(min_length);
  builder.ExportToSTL(out);
}
int main(int argc, char** argv) {
  if (argc != 4) return 2;
  FILE* in = fopen(argv[2], "rb");
  FILE* out = fopen(argv[3], "wb");
  if (!in || !out) return 1;
  uint32_t n_cases = 0;
  if (!get(in, &n_cases, 4)) return 1;
  for (uint32_t c = 0; c < n_cases; ++c) {
    matching::PairWiseMatches matches;
    if (!read_case(in, matches)) return 1;
    if (strcmp(argv[1], "time") == 0) {
      std::vector<double> ms;
      size_t n_tracks = 0;
      for (int r = 0; r < 5; ++r) {
        tracks::STLMAPTracks map_tracks;
        const auto t0 = std::chrono::steady_clock::now();
        run(matches, 2, map_tracks);
        ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        n_tracks = map_tracks.size();
      }
      std::sort(ms.begin(), ms.end());
      const double median = ms[2];
      const uint64_t n = n_tracks;
      put(out, &median, 8); put(out, &n, 8);
      continue;
    }
    for (uint32_t min_length = 2; min_length <= 3; ++min_length) {
      tracks::STLMAPTracks map_tracks;
      run(matches, min_length, map_tracks);
      const uint32_t n_tracks = (uint32_t)map_tracks.size();
      put(out, &n_tracks, 4);
      for (const auto& t : map_tracks) {
        const uint32_t head[2] = {t.first, (uint32_t)t.second.size()};
        put(out, head, 8);
        for (const auto& o : t.second) { const uint32_t v[2] = {o.first, o.second}; put(out, v, 8); }
      }
    }
  }
  fclose(out);
  return 0;
}
"""


def compile_driver(tmp):
    open(os.path.join(tmp, "driver.cpp"), "w").write(DRIVER)
    subprocess.run(["g++", "-O2", "-std=c++17", "-w", "-DEIGEN_MPL2_ONLY", "-I" + SRC, "-I" + os.path.join(SRC, "third_party", "eigen"), "-I" + os.path.join(SRC, "third_party"),
                    "-I" + os.path.join(SRC, "dependencies", "cereal", "include"), os.path.join(tmp, "driver.cpp"), "-o", os.path.join(tmp, "driver")], check=True)
    return os.path.join(tmp, "driver")


def write_cases(path, cases):
    with open(path, "wb") as f:
        f.write(np.uint32(len(cases)).tobytes())
        for c in cases:
            pairs, start, ij = np.asarray(c["pairs"], np.uint32).reshape(-1, 2), np.asarray(c["match_start"], np.int64), np.asarray(c["ij"], np.uint32).reshape(-1, 2)
            f.write(np.uint32(len(pairs)).tobytes())
            for p in range(len(pairs)):
                lo, hi = int(start[p]), int(start[p + 1])
                f.write(np.array([pairs[p, 0], pairs[p, 1], hi - lo], np.uint32).tobytes() + np.ascontiguousarray(ij[lo:hi]).tobytes())


def run_reference(cases):
    with tempfile.TemporaryDirectory() as tmp:
        exe = compile_driver(tmp)
        a, b = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        write_cases(a, cases)
        subprocess.run([exe, "tracks", a, b], check=True)
        raw = np.frombuffer(open(b, "rb").read(), np.uint32)
    at, out = 0, []
    for _ in cases:
        per = {}
        for ml in (2, 3):
            n_t = int(raw[at]); at += 1
            ids, lens, images, features = [], [], [], []
            for _t in range(n_t):
                ids.append(int(raw[at])); lens.append(int(raw[at + 1])); at += 2
                obs = raw[at:at + 2 * lens[-1]].reshape(-1, 2); at += 2 * lens[-1]
                images.append(obs[:, 0]); features.append(obs[:, 1])
            cat = lambda v: np.concatenate(v).astype(np.uint32) if v else np.zeros(0, np.uint32)   # noqa: E731
            per[ml] = dict(track_id=np.array(ids, np.uint32), track_len=np.array(lens, np.uint32), obs_image=cat(images), obs_feature=cat(features))
        out.append(per)
    assert at == len(raw)
    return out


def time_reference(directory):
    case = dict(pairs=np.load(os.path.join(directory, "pairs.npy")), match_start=np.load(os.path.join(directory, "match_start.npy")),
                ij=np.load(os.path.join(directory, "ij.npy")))
    with tempfile.TemporaryDirectory() as tmp:
        exe = compile_driver(tmp)
        a, b = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        write_cases(a, [case])
        subprocess.run([exe, "time", a, b], check=True)
        raw = open(b, "rb").read()
    print(json.dumps(dict(reference_ms=float(np.frombuffer(raw, np.float64, 1)[0]), n_tracks=int(np.frombuffer(raw, np.uint64, 1, 8)[0]), n_matches=int(len(case["ij"])),
                          n_pairs=int(len(case["pairs"])))))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--time":
        time_reference(sys.argv[2])
        sys.exit(0)
    cases = tref.fixture_cases()
    gold = run_reference(cases)
    n_collision = n_short_at_3_only = n_other_root = n_tracks = 0
    for c, per in zip(cases, gold):
        own = {ml: tref.build(c["pairs"], c["match_start"], c["ij"], None, ml) for ml in (2, 3)}
        for ml in (2, 3):
            assert np.array_equal(own[ml].track_id, per[ml]["track_id"]), (c["name"], ml, "track_id")
            assert np.array_equal(np.diff(own[ml].track_start.astype(np.int64)), per[ml]["track_len"]), (c["name"], ml, "lengths")
            assert np.array_equal(own[ml].obs_image, per[ml]["obs_image"]) and np.array_equal(own[ml].obs_feature, per[ml]["obs_feature"]), (c["name"], ml, "observations")
        n_collision += own[2].counts["n_collision"]
        n_short_at_3_only += own[3].counts["n_short"] - own[2].counts["n_short"]
        n_other_root += int((own[2].track_id != own[2].first_node).sum())
        n_tracks += len(own[2].track_id)
    print(len(cases), "cases,", n_tracks, "tracks at min_length 2;", n_collision, "colliding components,", n_short_at_3_only, "dropped for length at 3 alone,",
          n_other_root, "tracks whose id is not their first node")
    assert n_collision > 0 and n_short_at_3_only > 0 and n_other_root > 0
    assert any(c["n_features"] is not None for c in cases) and any(c["n_features"] is None and c["ij"].size and int(c["ij"].max()) > 60000 for c in cases)
    assert any(c["n_images"] > int(c["pairs"].max()) + 1 for c in cases if len(c["pairs"]))   # an image without any match
    cat = lambda key, dt: (np.concatenate([np.asarray(c[key], dt).reshape(-1) for c in cases]))   # noqa: E731
    arrays = dict(case_n_images=np.array([c["n_images"] for c in cases], np.uint32), case_n_pairs=np.array([len(c["pairs"]) for c in cases], np.uint32),
                  case_has_n_features=np.array([c["n_features"] is not None for c in cases]),
                  n_features=np.concatenate([c["n_features"] for c in cases if c["n_features"] is not None]).astype(np.uint32),
                  pairs=cat("pairs", np.uint32).reshape(-1, 2), match_start=cat("match_start", np.uint64), ij=cat("ij", np.uint32).reshape(-1, 2))
    for ml in (2, 3):
        arrays[f"n_tracks_{ml}"] = np.array([len(per[ml]["track_id"]) for per in gold], np.uint32)
        for k in ("track_id", "track_len", "obs_image", "obs_feature"):
            arrays[f"{k}_{ml}"] = np.concatenate([per[ml][k] for per in gold]).astype(np.uint32)
    # a fixed archive: members in this order, stored time zero - the same bytes from the same cases
    import io
    import zipfile
    with zipfile.ZipFile(GOLD_PATH, "w", zipfile.ZIP_DEFLATED) as z:
        for name, value in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(value), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), compress_type=zipfile.ZIP_DEFLATED)
    print(os.path.getsize(GOLD_PATH), "bytes")
