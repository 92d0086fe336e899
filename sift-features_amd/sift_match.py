"""sift-match: the counterpart of the crate's examples/sift-match.rs on the
MI355X path.

    python sift-features_amd/sift_match.py <a.jpg> <b.jpg> [--ratio R] [--verify [THR]]
                                           [--model homography|fundamental] [--progressive] [--guided]
                                           [--spread N]
                                           [--processing opencv|imageproc] [--device N]

examples/sift-match.rs:30-35, :87-97 opens two images, runs `sift()` on each and
matches the second's descriptors (query) against the first's (train) with
cv::BFMatcher(NORM_L2, crossCheck = true); it then draws the matches, which
this counterpart does not.  Here both JPEGs are decoded by the context's
decoder (jpeg.hip), `sift()` runs on the GPU through the C ABI and the
matcher is the MFMA kernel of match.hip.  Prints both keypoint counts and the
number of cross-checked matches.  `--ratio R` (0 < R <= 1) adds Lowe's ratio
test on the two nearest neighbours, a labelled extension (the crate has
none).  `--verify [THR]` (default 3 px), another labelled extension, fits a
RANSAC homography to the matches (verify.hip, the defaults of
Context.verify_matches) and prints a fourth line with its inlier count;
with `--model fundamental` (only read with --verify) it fits a RANSAC
fundamental matrix instead (verify_epipolar.hip; THR is the Sampson distance).
`--progressive` (only read with --verify), a labelled extension too, draws the
RANSAC samples in the order of the matches' descriptor distance (PROSAC:
Context.verify_matches(sampling="progressive")) and says so on the fourth line.
`--guided` (only read with --verify), a further labelled extension, matches
the pair again under the fitted model (match_guided.hip, the defaults of
Context.match_guided: cross check, no ratio test, no distance cap, the
verification's threshold) and prints a fifth line with the guided match count.
`--spread N`, a labelled extension as well, keeps at most N keypoints of each
image, spread over the frame by adaptive non-maximal suppression (select.hip,
the defaults of Context.select_keypoints), before matching; a further line
gives the kept counts, and the matches, inliers and guided matches are those
of the kept keypoints (their indices mapped back to the extraction's rows).
Exits non-zero (with the library's error) when the HIP library or
the device is missing: there is no CPU fallback.
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def main(argv=None):
    ap = argparse.ArgumentParser(prog="sift-match", description=__doc__.split("\n\n")[0])
    ap.add_argument("path_a")
    ap.add_argument("path_b")
    ap.add_argument("--ratio", type=float, default=None)
    ap.add_argument("--verify", type=float, nargs="?", const=3.0, default=None, metavar="THR")
    ap.add_argument("--model", choices=["homography", "fundamental"], default="homography")
    ap.add_argument("--progressive", action="store_true")
    ap.add_argument("--guided", action="store_true")
    ap.add_argument("--spread", type=int, default=None, metavar="N")
    ap.add_argument("--processing", choices=("imageproc", "opencv"), default="imageproc")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    import pkg_loader
    pkg = pkg_loader.load()
    proc = pkg.ImageprocProcessing if a.processing == "imageproc" else pkg.OpenCVProcessing
    datas = []
    for path in (a.path_a, a.path_b):
        with open(path, "rb") as f:
            datas.append(f.read())
    ctx = pkg.Context(a.device, proc)
    try:
        res_a, res_b = (ctx.sift_jpeg(d) for d in datas)
        kps_a, desc_a, kps_b, desc_b = res_a.keypoints_array, res_a.descriptors, res_b.keypoints_array, res_b.descriptors
        if a.spread is not None:
            rows_a, rows_b = (ctx.select_keypoints(k, a.spread)[0] for k in (kps_a, kps_b))
            kps_a, desc_a, kps_b, desc_b = kps_a[rows_a], desc_a[rows_a], kps_b[rows_b], desc_b[rows_b]
        qi, ti, dist = ctx.match_descriptors(desc_b, desc_a, cross_check=True, ratio=a.ratio)
        if a.verify is not None:
            g, _, info = ctx.verify_matches(kps_b, kps_a, (qi, ti, dist), threshold=a.verify, model=a.model,
                                            sampling="progressive" if a.progressive else "uniform")
            if a.guided:
                guided = ctx.match_guided(desc_b, kps_b, desc_a, kps_a, g, threshold=a.verify, model=a.model)
        if a.spread is not None:  # back to the rows of the two extractions
            qi, ti = rows_b[qi], rows_a[ti]
            if a.verify is not None and a.guided:
                guided = (rows_b[guided[0]], rows_a[guided[1]], *guided[2:])
    finally:
        ctx.close()
    print(f"{len(res_a)} keypoints")
    print(f"{len(res_b)} keypoints")
    if a.spread is not None:
        print(f"{len(rows_a)} and {len(rows_b)} kept (spread {a.spread})")
    print(f"{len(qi)} matches" + (f" (ratio {a.ratio:g})" if a.ratio is not None else ""))
    if a.verify is not None:
        print(f"{info['n_inliers']} inliers ({a.model}, threshold {a.verify:g}" +
              (", progressive)" if a.progressive else ")"))
        if a.guided:
            print(f"{len(guided[0])} guided matches")
    return 0


if __name__ == "__main__":
    sys.exit(main())
