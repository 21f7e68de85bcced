"""Paired evaluation on the HIP path: inference and scoring in one pass, the role of the reference's validation
(basicsr/models/image_restoration_model.py:564-711, :713-893 with options/train/FDN.yml: the ground-truth ratio, tensor2img, then
calculate_psnr / calculate_ssim on the 8-bit images), without the training framework around it:

    decode (PIL, worker threads) -> uint8 on the GPU -> fdn_pre_u8 -> ratio -> FDN -> fdn_post_u8 -> PSNR / SSIM against the ground truth

--ratio gt feeds FDN mean(gray(lq)) / mean(gray(gt)) as the validation does (:650-654; no LPNet needed), --ratio lpnet the ratio the
inference drivers feed (LPNet's prediction for --variant lolblur, mean(gray) / prediction for lolv1), --ratio VALUE that number for every
frame.  --bracket EV[,EV...] scores the exposure fusion (fdn_hip.fusion) of every frame's renderings at that ratio times 2^-EV per stop,
weighted with the exponents --fusion-weights C,S,E (inference_fdn_lolblur.py has what they mean; not what the reference scores).  --lq and --gt are globs, sorted
and paired by index; frames of equal size are batched and decoded one batch ahead.  The frames leave the GPU only with --output; the
scores take one small copy per batch.  Needs a ROCm GPU and the built libfdn_hip.so; there is no CPU fallback.

    python validate_fdn.py --fdn FDN_lolblur.pth --lq 'lolblur/test/low_blur/*/*' --gt 'lolblur/test/high_sharp_scaled/*/*' --csv scores.csv

--tile HxW plays the reference's `val.grids` with crop_size_h / crop_size_w (:261-339, :737-743): every frame is cut into overlapping tiles,
the ratio is taken per tile as the reference does after grids() (--tile-ratio tile, the default here; frame: one ratio from the whole
frame), and the merged 8-bit frame is scored.  The csv then holds one ratio per tile, joined by ';'.  --tile-blend feather merges the
tiles with ramps across their overlaps instead of the reference's average (not what the reference scores).  --ensemble 2|4|8 scores the
geometric self-ensemble (fdn_hip.ensemble; not what the reference scores either): FDN on that many flipped / transposed copies of every
frame or tile, all fed the ratio of the untransformed one, averaged.  --fourier appends the Fourier figures of fdn_hip.spectral to every
line and to the csv (calculate_fourier_metrics.py has what they mean): the amplitude, phase and zero-frequency share of the MSE of the whole
8-bit frame (no crop_border; the width must be even), the reference's FFTLoss, and per band the columns of that tool's csv.  --lowlight appends the two low-light scores of fdn_hip.lowlight
(calculate_lowlight_metrics.py has what they mean): loe, the lightness order error of the input frame against the restored one on a grid of
--loe-size points along the short side (0: every pixel), and deltae, the mean CIEDE2000 difference of the restored frame against the
ground truth, both from the whole 8-bit frames the driver holds on the GPU anyway.  --correct gt_mean|mean_var prints, beside the plain
scores, the PSNR and SSIM of the restored frame after that brightness correction towards the ground truth (calculate_psnr_ssim.py has
what the two mean): a wrong ratio costs the plain scores and not these.  A frame without a correction scores nan there; it is named on
stderr and the exit status is 1.  --sharpness appends the three deblurring figures of fdn_hip.sharpness (calculate_sharpness_metrics.py has what
they mean): edge, the reference's EdgeLoss of the restored frame against the ground truth, gmsd, and grad_ratio, the mean gradient
magnitude of the restored frame over that of the ground truth (below 1: softer than the truth), from the whole 8-bit frames.
--ms-ssim appends the multi-scale SSIM of fdn_hip.msssim (calculate_ms_ssim.py has what it means): the mean over R, G and B of the
five-scale score of the whole restored 8-bit frame against the ground truth; frames below 161 pixels in either side are refused.
--piqe appends the no-reference PIQE of fdn_hip.piqe (calculate_piqe.py has what it means; 0 best, 100 worst) of the whole restored
8-bit frame and, beside it, that of the ground truth, so that the two can be read side by side.
"""
import argparse
import glob
import os
import sys
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from calculate_psnr_ssim import decoded_groups  # noqa: E402

RATIO_MODE = {("gt", "lolblur"): "gt", ("gt", "lolv1"): "gt", ("lpnet", "lolblur"): "lolblur", ("lpnet", "lolv1"): "lolv1"}


def pair_frames(lq_glob, gt_glob):
    """sorted(glob(lq)) and sorted(glob(gt)), paired by index -> [(lq, gt)]"""
    lq, gt = sorted(glob.glob(lq_glob)), sorted(glob.glob(gt_glob))
    if not lq:
        raise ValueError(f"no input frames match {lq_glob!r}")
    if len(lq) != len(gt):
        raise ValueError(f"{len(lq)} input frames ({lq_glob!r}) but {len(gt)} ground-truth frames ({gt_glob!r})")
    return list(zip(lq, gt))


def output_paths(lq_paths, output):
    """a frame <common parent>/0256/0089.png is written to <output>/0256/0089.png, as the inference drivers keep the sequence folders"""
    root = os.path.commonpath([os.path.dirname(os.path.abspath(p)) for p in lq_paths])
    dest = [os.path.join(output, os.path.relpath(os.path.abspath(p), root)) for p in lq_paths]
    if len(set(dest)) != len(dest):
        raise ValueError("two input frames map to the same output path")
    return dest


def ratio_arg(s):
    """--ratio: gt, lpnet, or a number"""
    if s in ("gt", "lpnet"):
        return s
    from inference_fdn_lolblur import ratio_value
    try:
        return ratio_value(s)
    except argparse.ArgumentTypeError:
        raise argparse.ArgumentTypeError(f"{s!r}: gt, lpnet or a finite number")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--fdn", required=True, help="FDN checkpoint ({'params': state_dict})")
    ap.add_argument("--lpnet", default=None, help="LPNet checkpoint; needed with --ratio lpnet only")
    ap.add_argument("--lq", required=True, help="low-quality input frames: a glob, sorted")
    ap.add_argument("--gt", required=True, help="ground-truth frames: a glob, sorted and paired with --lq by index")
    ap.add_argument("--variant", choices=("lolblur", "lolv1"), default="lolblur", help="FDN (dim 32) or FDN_lolv1 (dim 24)")
    ap.add_argument("--ratio", type=ratio_arg, default="gt", metavar="gt|lpnet|VALUE",
                    help="where ratio_i comes from: the ground truth (validation), LPNet, or this number for every frame")
    ap.add_argument("--crop_border", type=int, default=0, help="pixels cut from every edge before scoring")
    ap.add_argument("--output", default=None, help="directory for the restored frames; without it no frame is written")
    ap.add_argument("--csv", default=None, help="file for one 'frame,psnr,ssim,ratio' line per pair")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--device", default="cuda:0")
    from inference_fdn_lolblur import add_ensemble_arg, add_tile_args, bracket_arg, fusion_weights_arg, glue_bracket
    add_tile_args(ap, ratio_default="tile")
    add_ensemble_arg(ap)
    # absent unless given, as the flags below
    ap.add_argument("--bracket", type=bracket_arg, default=argparse.SUPPRESS, metavar="EV[,EV...]",
                    help="score the exposure fusion of every frame's renderings at its ratio times 2^-EV for each of these stops")
    ap.add_argument("--fusion-weights", type=fusion_weights_arg, default=argparse.SUPPRESS, metavar="C,S,E",
                    help="with --bracket: the exponents of contrast, saturation and well-exposedness (default 1,1,1)")
    ap.add_argument("--fourier", action="store_true", help="also split every frame's error into amplitude and phase per frequency band")
    ap.add_argument("--fourier-bands", type=int, default=8, help="radial frequency bands besides the zero-frequency bin (1 .. 32)")
    # absent unless given, so that the namespace of a command line without them is what it was
    ap.add_argument("--lowlight", action="store_true", default=argparse.SUPPRESS,
                    help="also score the lightness order error against the input and the CIEDE2000 difference against the ground truth")
    ap.add_argument("--loe-size", type=int, default=argparse.SUPPRESS, help="with --lowlight: points along the short side of LOE's sample grid (default 50; 0 = full resolution)")
    ap.add_argument("--correct", choices=("gt_mean", "mean_var"), default=argparse.SUPPRESS,
                    help="also score every frame after a brightness correction towards the ground truth (fdn_hip.correct)")
    ap.add_argument("--sharpness", action="store_true", default=argparse.SUPPRESS,
                    help="also score the edge error, GMSD and the mean-gradient ratio against the ground truth (fdn_hip.sharpness)")
    ap.add_argument("--ms-ssim", action="store_true", default=argparse.SUPPRESS,
                    help="also score the multi-scale SSIM (rgb) against the ground truth (fdn_hip.msssim; frames of at least 161x161)")
    ap.add_argument("--piqe", action="store_true", default=argparse.SUPPRESS,
                    help="also score the no-reference PIQE of the restored frame and of the ground truth (fdn_hip.piqe)")
    a = ap.parse_args(glue_bracket(argv))
    if not 1 <= a.fourier_bands <= 32:
        ap.error("--fourier-bands must be in 1 .. 32")
    if hasattr(a, "loe_size") and not hasattr(a, "lowlight"):
        ap.error("--loe-size needs --lowlight")
    if getattr(a, "loe_size", 0) < 0:
        ap.error("--loe-size must be >= 0")
    if hasattr(a, "fusion_weights") and not hasattr(a, "bracket"):
        ap.error("--fusion-weights needs --bracket")
    if a.ratio == "lpnet" and not a.lpnet:
        ap.error("--ratio lpnet needs --lpnet")
    if a.crop_border < 0:
        ap.error("--crop_border must be >= 0")
    try:
        a.pairs = pair_frames(a.lq, a.gt)
        a.dest = output_paths([p for p, _ in a.pairs], a.output) if a.output else None
    except ValueError as e:
        ap.error(str(e))
    return a


def csv_header(a):
    """the first line of --csv: columns are added only by the flags that are given"""
    cols = "frame,psnr,ssim,ratio"
    if a.fourier:
        from fdn_hip import spectral
        cols += "," + ",".join(spectral.csv_header(a.fourier_bands))
    return cols + (",loe,deltae" if getattr(a, "lowlight", False) else "") + (",psnr_corr,ssim_corr" if getattr(a, "correct", None) else "") + (
        ",edge,gmsd,grad_ratio" if getattr(a, "sharpness", False) else "") + (",ms_ssim" if getattr(a, "ms_ssim", False) else "") + (
        ",piqe,piqe_gt" if getattr(a, "piqe", False) else "")


def main(argv=None):
    a = parse_args(argv)
    import torch
    from fdn_hip.harness import validate_u8
    from inference_fdn_lolblur import hint_hard_seam, hint_large_frame, load_params, write_rgb
    from basicsr.models.archs.LPNet_arch import I_predict_net
    if a.variant == "lolblur":
        from basicsr.models.archs.FDN_arch import FDN as Net
    else:
        from basicsr.models.archs.fdnlol24_arch import FDN_lolv1 as Net

    if a.fourier:
        from calculate_fourier_metrics import SUMMARY_KEYS, fourier_line, mean_of
        from fdn_hip import FdnHipError, spectral

    want_ll, loe_size = getattr(a, "lowlight", False), getattr(a, "loe_size", 50)
    if want_ll:
        from calculate_lowlight_metrics import lowlight_line
        from fdn_hip import FdnHipError, lowlight

    mode_corr = getattr(a, "correct", None)
    want_sh = getattr(a, "sharpness", False)
    if want_sh:
        from calculate_sharpness_metrics import sharpness_line
        from fdn_hip import FdnHipError, sharpness
    want_ms = getattr(a, "ms_ssim", False)
    if want_ms:
        from fdn_hip import FdnHipError, msssim
    want_pq = getattr(a, "piqe", False)
    if want_pq:
        from fdn_hip import FdnHipError, piqe

    dev = torch.device(a.device)
    torch.cuda.set_device(dev)
    net = Net().to(dev).eval()
    net.load_state_dict(load_params(a.fdn), strict=True)
    lp = None
    if a.ratio == "lpnet":
        lp = I_predict_net().to(dev).eval()
        lp.load_state_dict(load_params(a.lpnet), strict=True)
    fixed = not isinstance(a.ratio, str)
    mode = "fixed" if fixed else RATIO_MODE[(a.ratio, a.variant)]
    more = {"correct": mode_corr} if mode_corr else {}
    if hasattr(a, "bracket"):
        more.update(bracket=a.bracket, fusion=getattr(a, "fusion_weights", (1.0, 1.0, 1.0)))

    n = len(a.pairs)
    psnr, ssim, ratio, fourier, ll, corr, sh = [None] * n, [None] * n, [None] * n, [None] * n, [None] * n, [None] * n, [None] * n
    mss, pq = [None] * n, [None] * n
    with ThreadPoolExecutor(max_workers=4) as pool:
        writers = []
        for idx, lqs, gts in decoded_groups(a.pairs, a.batch, pool):
            lq, gt = torch.from_numpy(lqs).to(dev), torch.from_numpy(gts).to(dev)
            hint_large_frame(a.tile, lqs.shape[1], lqs.shape[2])
            hint_hard_seam(a.tile, a.tile_blend, a.tile_overlap, lqs.shape[1], lqs.shape[2])
            out, p, s, r, *pc = validate_u8(net, lp, lq, gt, ratio_mode=mode, crop_border=a.crop_border, bgr=False, tile=a.tile,
                                            ratio_from=a.tile_ratio, overlap=a.tile_overlap, batch=a.batch, blend=a.tile_blend,
                                            ensemble=a.ensemble, **more,
                                            **({"ratio": torch.full((lq.shape[0], 1), a.ratio, dtype=torch.float32, device=dev)} if fixed else {}))
            r = r.reshape(r.shape[0], -1).cpu().tolist()              # one ratio per frame, or one per tile of a tiled frame
            frames = out.cpu().numpy() if a.dest else None
            if a.fourier:
                try:
                    fm = spectral.calculate_fourier(out, gt, bands=a.fourier_bands, bgr=False)
                except FdnHipError as e:
                    sys.exit(f"validate_fdn.py: --fourier: {e}")
            if want_ll:
                try:
                    lm = lowlight.lowlight_metrics(lq, out, gt, size=loe_size, bgr=False)
                except FdnHipError as e:
                    sys.exit(f"validate_fdn.py: --lowlight: {e}")
            if want_sh:
                try:
                    sm = sharpness.sharpness_metrics(gt, out, bgr=False)
                except FdnHipError as e:
                    sys.exit(f"validate_fdn.py: --sharpness: {e}")
            if want_ms:
                try:
                    mm = msssim.ms_ssim_u8(gt, out, mode="rgb", bgr=False)
                except FdnHipError as e:
                    sys.exit(f"validate_fdn.py: --ms-ssim: {e}")
            if want_pq:
                try:
                    pm, pg = piqe.piqe_u8(out, bgr=False), piqe.piqe_u8(gt, bgr=False)
                except FdnHipError as e:
                    sys.exit(f"validate_fdn.py: --piqe: {e}")
            for k, i in enumerate(idx):
                psnr[i], ssim[i], ratio[i] = p[k], s[k], r[k]
                if a.fourier:
                    fourier[i] = fm[k]
                if want_ll:
                    ll[i] = lm[k]
                if mode_corr:
                    corr[i] = (pc[0][k], pc[1][k])
                if want_sh:
                    sh[i] = sm[k]
                if want_ms:
                    mss[i] = mm[k]["ms_ssim"]
                if want_pq:
                    pq[i] = (pm[k]["piqe"], pg[k]["piqe"])
                if a.dest:
                    writers.append(pool.submit(write_rgb, a.dest[i], frames[k]))
        for w in writers:
            w.result()
    for i, (lq_path, _) in enumerate(a.pairs):
        basename = os.path.splitext(os.path.basename(lq_path))[0]
        tail = f", \t{fourier_line(fourier[i])}" if a.fourier else ""
        tail += f", \t{lowlight_line(ll[i])}" if want_ll else ""
        tail += f", \t{mode_corr} PSNR: {corr[i][0]:.6f} dB, \t{mode_corr} SSIM: {corr[i][1]:.6f}" if mode_corr else ""
        tail += f", \t{sharpness_line(sh[i])}" if want_sh else ""
        tail += f", \tMS-SSIM: {mss[i]:.6f}" if want_ms else ""
        tail += f", \tPIQE: {pq[i][0]:.6f} (gt {pq[i][1]:.6f})" if want_pq else ""
        print(f'{i+1:3d}: {basename:25}. \tPSNR: {psnr[i]:.6f} dB, \tSSIM: {ssim[i]:.6f}{tail}')
    tail = ", " + fourier_line({k: mean_of([m[k] for m in fourier]) for k in SUMMARY_KEYS}) if a.fourier else ""
    tail += ", " + lowlight_line({k: sum(m[k] for m in ll) / n for k in ("loe", "deltae")}) if want_ll else ""
    tail += f", {mode_corr} PSNR: {sum(c[0] for c in corr) / n:.6f} dB, {mode_corr} SSIM: {sum(c[1] for c in corr) / n:.6f}" if mode_corr else ""
    tail += ", " + sharpness_line({k: sum(m[k] for m in sh) / n for k in ("edge", "gmsd", "grad_ratio")}) if want_sh else ""
    tail += f", MS-SSIM: {sum(mss) / n:.6f}" if want_ms else ""
    tail += f", PIQE: {sum(q[0] for q in pq) / n:.6f} (gt {sum(q[1] for q in pq) / n:.6f})" if want_pq else ""
    print(f'Average: PSNR: {sum(psnr) / n:.6f} dB, SSIM: {sum(ssim) / n:.6f}{tail}')
    if a.csv:
        os.makedirs(os.path.dirname(a.csv) or ".", exist_ok=True)
        with open(a.csv, "w") as f:
            f.write(csv_header(a) + "\n")
            for i, ((lq_path, _), p, s, r) in enumerate(zip(a.pairs, psnr, ssim, ratio)):
                tail = "," + ",".join(spectral.csv_row(fourier[i])) if a.fourier else ""
                tail += f",{ll[i]['loe']!r},{ll[i]['deltae']!r}" if want_ll else ""
                tail += f",{corr[i][0]!r},{corr[i][1]!r}" if mode_corr else ""
                tail += f",{sh[i]['edge']!r},{sh[i]['gmsd']!r},{sh[i]['grad_ratio']!r}" if want_sh else ""
                tail += f",{mss[i]!r}" if want_ms else ""
                tail += f",{pq[i][0]!r},{pq[i][1]!r}" if want_pq else ""
                f.write(f"{lq_path},{p!r},{s!r},{';'.join(repr(v) for v in r)}{tail}\n")
    if a.dest:
        print(f"{n} frames -> {a.output}")
    bad = [lq_path for (lq_path, _), c in zip(a.pairs, corr) if mode_corr and (c[0] != c[0] or c[1] != c[1])]
    for path in bad:
        print(f"validate_fdn.py: --correct {mode_corr}: the restored {path} has no correction (a flat channel or a black image): nan", file=sys.stderr)
    if bad:
        sys.exit(1)


if __name__ == "__main__":
    main()
