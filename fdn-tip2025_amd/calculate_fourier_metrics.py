"""The error of restored images against their ground truth, split in the Fourier domain on the HIP path (fdn_hip.spectral): how much of
the MSE behind PSNR is an amplitude error (brightness, exposure) and how much a phase error (structure, blur), per radial frequency band,
and the FFT term of the loss the reference trains with (FFTLoss of basicsr/models/losses/losses.py, 'mean' reduction).  Both globs are
sorted and paired by index, as calculate_psnr_ssim.py pairs them; pairs of equal size are scored as one batch.  Needs a ROCm GPU and the
built libfdn_hip.so; there is no CPU fallback.  Images must be 8-bit RGB of even width.

    python calculate_fourier_metrics.py --gt 'lolblur/test/high_sharp_scaled/*/*' --restored 'results/lolblur/*/*' --csv fourier.csv

One line per pair: PSNR, the amplitude, phase and zero-frequency (DC) share of the MSE, fft_l1; then the averages.  --csv adds, per band,
the band's share of the MSE, its amplitude and phase part and its error relative to the ground truth's energy in the band.  Band 0 is
the zero-frequency bin alone; bands 1 .. N cut the radial frequency at multiples of 0.5 / N cycles per pixel.
"""
import argparse
import os
import sys
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from calculate_lpips import pair_paths  # noqa: E402
from calculate_psnr_ssim import decoded_groups  # noqa: E402

SUMMARY_KEYS = ("psnr", "amp_share", "pha_share", "dc_share", "fft_l1")


def score_pairs(pairs, bands=8, batch=8, device="cuda:0", workers=4):
    """-> one dict of fdn_hip.spectral.metrics_from_sums per (gt, restored) pair, in order"""
    import torch
    from fdn_hip import spectral
    dev = torch.device(device)
    torch.cuda.set_device(dev)
    out = [None] * len(pairs)
    with ThreadPoolExecutor(max_workers=workers) as pool:
        for idx, gts, rss in decoded_groups(pairs, batch, pool):
            res = spectral.calculate_fourier(torch.from_numpy(rss).to(dev), torch.from_numpy(gts).to(dev), bands=bands, bgr=False)
            for k, i in enumerate(idx):
                out[i] = res[k]
    return out


def fourier_line(m):
    """the Fourier figures of one pair, as printed here and by validate_fdn.py --fourier"""
    return f"Amp: {m['amp_share']:.6f}, Pha: {m['pha_share']:.6f}, DC: {m['dc_share']:.6f}, FFT-L1: {m['fft_l1']:.6f}"


def mean_of(values):
    """the mean of the values that are numbers (two equal images have no shares: nan); nan when none is"""
    v = [x for x in values if x == x]
    return sum(v) / len(v) if v else float("nan")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gt", required=True, help="ground-truth images: a glob, sorted")
    ap.add_argument("--restored", required=True, help="restored images: a glob, sorted and paired with --gt by index")
    ap.add_argument("--bands", type=int, default=8, help="radial frequency bands besides the zero-frequency bin (1 .. 32)")
    ap.add_argument("--csv", default=None, help="file for one line per pair with the per-band columns")
    ap.add_argument("--batch", type=int, default=8, help="pairs of equal size scored per launch")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    if not 1 <= a.bands <= 32:
        ap.error("--bands must be in 1 .. 32")
    if a.batch < 1:
        ap.error("--batch must be >= 1")
    try:
        a.pairs = pair_paths(a.gt, a.restored)
    except ValueError as e:
        ap.error(str(e))
    return a


def main(argv=None):
    a = parse_args(argv)
    from fdn_hip import FdnHipError, spectral
    try:
        res = score_pairs(a.pairs, a.bands, a.batch, a.device)
    except FdnHipError as e:
        sys.exit(f"calculate_fourier_metrics.py: {e}")
    for i, ((gt, _), m) in enumerate(zip(a.pairs, res)):
        basename = os.path.splitext(os.path.basename(gt))[0]
        print(f"{i+1:3d}: {basename:25}. \tPSNR: {m['psnr']:.6f} dB, \t{fourier_line(m)}")
    avg = {k: mean_of([m[k] for m in res]) for k in SUMMARY_KEYS}
    print(f"Average: PSNR: {avg['psnr']:.6f} dB, {fourier_line(avg)}")
    if a.csv:
        os.makedirs(os.path.dirname(a.csv) or ".", exist_ok=True)
        with open(a.csv, "w") as f:
            f.write("gt,restored," + ",".join(spectral.csv_header(a.bands)) + "\n")
            for (gt, rs), m in zip(a.pairs, res):
                f.write(f"{gt},{rs}," + ",".join(spectral.csv_row(m)) + "\n")


if __name__ == "__main__":
    main()
