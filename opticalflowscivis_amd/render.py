"""Pictures of what the pipeline writes: a series of volumes (`reconstruct`'s frames, or a field of `ftle`, `vortex` or
`regions`) is ray-cast on the device through an orbiting camera and a transfer function (ops.raycast: emission /
absorption or maximum intensity, one launch per `--chunk` of frames); 2-D frames and fields are colour-mapped through the
same transfer function, and flows become the reference's `flow2rgb` pictures.  Shared by the flow2d / flow3d / upflow
`render` entry points:

    python -m opticalflowscivis_amd.flow3d.render --seq frames.npy --tf hot --range 0 1 --image 512 512 \
        --azimuth 30 --elevation 20 --orbit 3 --out img.npy --png-dir shots --json r.json
    python -m opticalflowscivis_amd.flow3d.render --field ftle.npy --tf iso:0.4 --mode dvr --fov 40 --png-dir shots
    python -m opticalflowscivis_amd.flow3d.render --field vg.npy --plane 2 --tf coolwarm --mode mip --out img.npy
    python -m opticalflowscivis_amd.flow2d.render --seq frames.npy --tf grey --flows flows.npy --png-dir shots

--field takes [K, *sp] or [K, NP, *sp] (--plane picks one of the NP planes).  --tf is a preset (grey, hot, coolwarm,
iso:<value>) or a [n, 4] .npy of RGBA rows spread over --range (default: the finite minimum and maximum of the data); a
row's A is an extinction per unit length, scaled by --opacity (default 8 / the volume's diagonal).  The camera looks at
the volume's centre from --azimuth / --elevation degrees (z up) and turns by --orbit degrees per frame; --fov makes it
a perspective camera, without it the projection is orthographic.  --out holds fp32 [K, rows, columns, 4] RGBA; --png-dir
gets one 8-bit RGBA PNG per frame (zlib and struct only); the JSON holds per frame its time (index * --dt), the mean
opacity and the samples taken.

Each chunk of frames is uploaded once, rendered by one launch (plus one for the brick ranges that let rays jump over
empty space; --no-bricks leaves it out -- the pictures are the same bit for bit) and dropped: device memory is one chunk
of volumes and of images.

Out of scope: gradient shading; depth output; label and categorical volumes; several fields in one picture; autograd; an
interactive viewer.  Isosurface extraction -- the geometry behind an `iso:<value>` picture, as triangle meshes -- is
opticalflowscivis_amd/isosurface.py (`flow3d.isosurface`)."""
import argparse
import math
import os
import struct
import time
import zlib

import numpy as np
import torch

from . import ops
from .stepflows import write_report

PRESETS = ("grey", "hot", "coolwarm", "iso:<value>")


# ---------------------------------------------------------------------------------------------------------------------
# camera
# ---------------------------------------------------------------------------------------------------------------------
def _extent(shape, spacing):
    sp = tuple(int(s) for s in shape)
    if len(sp) != 3 or min(sp) < 2:
        raise ValueError("shape must be (D,H,W) with every extent >= 2, got %r" % (shape,))
    hs = [float(v) for v in spacing] if hasattr(spacing, "__len__") else [float(spacing)] * 3
    if len(hs) != 3 or not all(0 < h < float("inf") for h in hs):
        raise ValueError("spacing must be one or 3 finite positive values (D,H,W), got %r" % (spacing,))
    # physical size along x, y, z: node i of an axis sits at i * spacing
    return np.array([(n - 1) * h for n, h in zip(sp[::-1], hs[::-1])], np.float64)


def camera_basis(azimuth, elevation):
    """(right, up, forward): an orthonormal basis for a camera that looks at the origin from `azimuth` degrees about z
    (from +x towards +y) and `elevation` degrees above the x-y plane; z is up (y when looking straight along z)."""
    az, el = math.radians(float(azimuth)), math.radians(float(elevation))
    eye = np.array([math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el)])
    fwd = -eye
    world_up = np.array([0.0, 0.0, 1.0]) if abs(eye[2]) < 1.0 - 1e-9 else np.array([0.0, 1.0, 0.0])
    right = np.cross(fwd, world_up)
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    return right, up / np.linalg.norm(up), fwd


def orbit_camera(shape, spacing, azimuth, elevation, distance, image, fov=None):
    """The 18 numbers (o, ou, ov, d, du, dv; float32) of a camera that looks at the centre of a volume of `shape`
    (D,H,W) nodes `spacing` apart from `distance` away: pixel (i, j) -- column i of row j of an `image` = (rows, columns)
    picture -- has the origin o + i ou + j ov and the direction normalize(d + i du + j dv).  fov=None: orthographic, the
    shorter side of the picture spans the volume's diagonal; fov: the vertical field of view in degrees of a perspective
    camera.  distance=None: 1.5 diagonals.  Row 0 is the top of the picture."""
    size = _extent(shape, spacing)
    Hi, Wi = (int(v) for v in image)
    if Hi < 1 or Wi < 1:
        raise ValueError("image must be (rows, columns) >= 1, got %r" % (image,))
    diag = float(np.linalg.norm(size))
    distance = 1.5 * diag if distance is None else float(distance)
    if not (0 <= distance < float("inf")):
        raise ValueError("distance must be finite and not negative, got %r" % (distance,))
    right, up, fwd = camera_basis(azimuth, elevation)
    eye = 0.5 * size - distance * fwd
    ci, cj = 0.5 * (Wi - 1), 0.5 * (Hi - 1)
    zero = np.zeros(3)
    if fov is None:
        s = diag / min(Hi, Wi)
        cam = [eye - ci * s * right + cj * s * up, s * right, -s * up, fwd, zero, zero]
    else:
        fov = float(fov)
        if not (0 < fov < 180):
            raise ValueError("fov must lie in (0, 180) degrees, got %r" % (fov,))
        s = 2.0 * math.tan(math.radians(fov) / 2.0) / Hi
        cam = [eye, zero, zero, fwd - ci * s * right + cj * s * up, s * right, -s * up]
    return np.concatenate(cam).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# transfer functions
# ---------------------------------------------------------------------------------------------------------------------
def _ramp(u, stops):
    """Piecewise linear colours: stops = [(position, (r, g, b)), ...] in increasing position."""
    pos = np.array([p for p, _ in stops])
    col = np.array([c for _, c in stops], np.float64)
    return np.stack([np.interp(u, pos, col[:, k]) for k in range(3)], -1)


def tf_preset(name, n=256, lo=0.0, hi=1.0, opacity=1.0):
    """A [n, 4] float32 RGBA table spread over the values [lo, hi]; A (an extinction per unit length) is scaled by
    `opacity`.  grey: black to white, A rising with the value.  hot: black, red, yellow, white, A rising.  coolwarm: blue,
    white, red, A = the distance from the middle.  iso:<value>: hot colours, A a narrow peak at <value> and 0 elsewhere
    -- most of a volume is then empty space."""
    n = int(n)
    if not 2 <= n <= ops.RC_MAX_TF:
        raise ValueError("a table has 2..%d rows, got %d" % (ops.RC_MAX_TF, n))
    u = np.linspace(0.0, 1.0, n)
    hot = [(0.0, (0, 0, 0)), (1 / 3, (1, 0, 0)), (2 / 3, (1, 1, 0)), (1.0, (1, 1, 1))]
    if name == "grey":
        rgb, a = np.stack([u, u, u], -1), u
    elif name == "hot":
        rgb, a = _ramp(u, hot), u
    elif name == "coolwarm":
        rgb = _ramp(u, [(0.0, (0.23, 0.30, 0.75)), (0.5, (0.87, 0.87, 0.87)), (1.0, (0.71, 0.02, 0.15))])
        a = np.abs(2.0 * u - 1.0)
    elif name.startswith("iso:"):
        try:
            v = float(name[4:])
        except ValueError:
            raise ValueError("iso:<value> needs a number, got %r" % (name,))
        p = (v - float(lo)) / (float(hi) - float(lo))
        w = max(2.0 / (n - 1), 0.02)
        rgb, a = _ramp(u, hot), np.maximum(0.0, 1.0 - np.abs(u - p) / w)
    else:
        raise ValueError("unknown transfer function %r: choose among %s or give a .npy" % (name, ", ".join(PRESETS)))
    return np.concatenate([rgb, (float(opacity) * a)[:, None]], -1).astype(np.float32)


def load_tf(spec, n=256, lo=0.0, hi=1.0, opacity=1.0):
    """tf_preset(spec, ...) or, when spec ends in .npy, the [n, 4] RGBA table of that file (A scaled by `opacity`)."""
    if not str(spec).endswith(".npy"):
        return tf_preset(str(spec), n, lo, hi, opacity)
    t = np.load(spec)
    if t.ndim != 2 or t.shape[1] != 4 or not 2 <= t.shape[0] <= ops.RC_MAX_TF:
        raise ValueError("%s must hold [n,4] RGBA rows, 2 <= n <= %d, got %s" % (spec, ops.RC_MAX_TF, t.shape))
    t = t.astype(np.float32)
    if not np.isfinite(t).all() or (t[:, 3] < 0).any():
        raise ValueError("%s must be finite with A >= 0" % spec)
    t[:, 3] *= np.float32(opacity)
    return t


# ---------------------------------------------------------------------------------------------------------------------
# pictures
# ---------------------------------------------------------------------------------------------------------------------
def to_uint8(img):
    """fp RGBA / RGB in [0, 1] -> uint8, rounded to nearest; what is not finite becomes 0."""
    a = np.nan_to_num(np.asarray(img, np.float32), nan=0.0, posinf=1.0, neginf=0.0)
    return np.rint(np.clip(a, 0.0, 1.0) * 255.0).astype(np.uint8)


def png_bytes(pixels):
    """An 8-bit PNG (grey [H,W], RGB [H,W,3] or RGBA [H,W,4] uint8) as bytes: zlib and struct only, filter 0 rows."""
    a = np.asarray(pixels)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] not in (3, 4)) or a.size == 0:
        raise ValueError("a PNG takes uint8 [H,W], [H,W,3] or [H,W,4], got %s %s" % (a.dtype, a.shape))
    h, w = a.shape[:2]
    colour = 0 if a.ndim == 2 else (2 if a.shape[2] == 3 else 6)
    rows = np.concatenate([np.zeros((h, 1), np.uint8), np.ascontiguousarray(a).reshape(h, -1)], 1)

    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xffffffff)

    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, colour, 0, 0, 0)) +
            chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + chunk(b"IEND", b""))


def write_png(path, pixels):
    with open(path, "wb") as f:
        f.write(png_bytes(pixels))


def flow2rgb(flow, base=0.0):
    """The reference's flow picture: flow [H, W, 2] -> float32 [H, W, 3] in [0, 1].  The flow is divided by its largest
    component magnitude; R = base + u, G = base - (u + v) / 2, B = base + v, clipped.  base 0 is the reference's shared
    utility (a black picture where nothing moves), base 1 its Flow-3D training script's variant (white)."""
    f = np.asarray(flow)
    if f.ndim != 3 or f.shape[2] != 2:
        raise ValueError("flow must be [H,W,2], got %s" % (f.shape,))
    rgb = np.full(f.shape[:2] + (3,), base, np.float32)
    nf = f / np.abs(f).max()
    rgb[:, :, 0] += nf[:, :, 0]
    rgb[:, :, 1] -= 0.5 * (nf[:, :, 0] + nf[:, :, 1])
    rgb[:, :, 2] += nf[:, :, 1]
    return rgb.clip(0, 1)


def colormap(values, tf, lo, hi):
    """values [...] (torch, any device) through the table: RGBA [..., 4] in stock torch ops -- the 2-D counterpart of the
    ray caster's lookup.  What is not finite becomes 0."""
    tf = torch.as_tensor(tf, dtype=torch.float32, device=values.device)
    n = tf.shape[0]
    v = values.to(torch.float32)
    fin = torch.isfinite(v)
    s = ((torch.where(fin, v, torch.full_like(v, lo)) - lo) * (1.0 / (hi - lo))).clamp(0.0, 1.0) * (n - 1)
    j = s.floor().long().clamp(max=n - 2)
    ft = (s - j.to(torch.float32))[..., None]
    return (tf[j] + ft * (tf[j + 1] - tf[j])) * fin[..., None].to(torch.float32)


# ---------------------------------------------------------------------------------------------------------------------
# series
# ---------------------------------------------------------------------------------------------------------------------
def render_series(volumes_of, n_frames, sp, cameras, tf, lo, hi, image, dt=None, spacing=1.0, mode="dvr", t_min=0.0,
                  chunk=4, bricks=True, times=None, keep_images=True):
    """Pictures of the n_frames volumes that volumes_of(j0, j1) -> fp32 [j1 - j0, D, H, W] on the device hands out
    `chunk` at a time (each exactly once; one ops.raycast launch per chunk, preceded by one ops.brick_ranges launch with
    bricks).  cameras: [n_frames, 18] or one camera; times: the time of every frame (default its index).

    Returns a dict: images (fp32 [n_frames, rows, columns, 4] in host memory; keep_images), frames (one dict per frame:
    frame, time, mean_opacity, samples -- the samples its rays gathered) and the totals time_load_s, time_kernel_s."""
    chunk = max(1, int(chunk))
    n_frames = int(n_frames)
    Hi, Wi = (int(v) for v in image)
    cams = np.asarray(cameras, np.float32)
    cams = np.broadcast_to(cams.reshape(-1, 18), (n_frames, 18)) if cams.size == 18 else cams.reshape(n_frames, 18)
    times = list(range(n_frames)) if times is None else [float(t) for t in times]
    if len(times) != n_frames:
        raise ValueError("times must name the %d frames, got %d" % (n_frames, len(times)))
    res = {}
    if keep_images:
        res["images"] = torch.empty((n_frames, Hi, Wi, 4), dtype=torch.float32)
    rows = []
    t_load = t_kernel = 0.0
    for j0 in range(0, n_frames, chunk):
        j1 = min(n_frames, j0 + chunk)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        v = volumes_of(j0, j1)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        br = ops.brick_ranges(v) if bricks else None
        r = ops.raycast(v, np.ascontiguousarray(cams[j0:j1]), tf, lo, hi, dt, spacing, mode, t_min, br, True, (Hi, Wi))
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        t_load += t1 - t0
        t_kernel += t2 - t1
        opacity = r["image"][..., 3].mean(dim=(1, 2)).cpu().tolist()
        samples = r["counts"].sum(dim=(1, 2), dtype=torch.int64).cpu().tolist()
        for j in range(j0, j1):
            rows.append({"frame": j, "time": times[j], "mean_opacity": opacity[j - j0], "samples": int(samples[j - j0])})
        if keep_images:
            res["images"][j0:j1].copy_(r["image"])
        del v, br, r
    res.update(frames=rows, time_load_s=t_load, time_kernel_s=t_kernel)
    return res


# ---------------------------------------------------------------------------------------------------------------------
# entry points
# ---------------------------------------------------------------------------------------------------------------------
def _args(nd, desc):
    sp = ",".join("DHW"[3 - nd:])
    ap = argparse.ArgumentParser(description=desc)
    ap.add_argument("--seq", help=".npy sequence [T,%s]" % sp)
    ap.add_argument("--field", help=".npy field [K,%s] or [K,NP,%s] as ftle, vortex and regions write them" % (sp, sp))
    ap.add_argument("--plane", type=int, default=0, help="the plane of a [K,NP,%s] --field" % sp)
    ap.add_argument("--tf", default="hot", help="%s, or a [n,4] RGBA .npy" % ", ".join(PRESETS))
    ap.add_argument("--tf-size", type=int, default=256, help="rows of a preset table")
    ap.add_argument("--range", type=float, nargs=2, default=None, metavar=("LO", "HI"),
                    help="the values the table spans (default: the data's finite minimum and maximum)")
    ap.add_argument("--dt", type=float, default=1.0, help="the time one frame spans: a frame's time is its index * dt")
    ap.add_argument("--out", default=None, metavar="IMG.npy", help="write the pictures [K, rows, columns, 4] (fp32) here")
    ap.add_argument("--png-dir", default=None, metavar="DIR", help="write frame_%%04d.png (8-bit RGBA) here")
    ap.add_argument("--json", default=None, help="write the report as JSON here")
    if nd == 3:
        ap.add_argument("--mode", choices=sorted(ops.RC_MODES), default="dvr")
        ap.add_argument("--image", type=int, nargs=2, default=[512, 512], metavar=("ROWS", "COLUMNS"))
        ap.add_argument("--azimuth", type=float, default=30.0, help="degrees about z, from +x towards +y")
        ap.add_argument("--elevation", type=float, default=20.0, help="degrees above the x-y plane")
        ap.add_argument("--orbit", type=float, default=0.0, metavar="DEG", help="turn the camera by DEG per frame")
        ap.add_argument("--fov", type=float, default=None, help="vertical field of view in degrees (default: orthographic)")
        ap.add_argument("--distance", type=float, default=None, help="eye to centre (default: 1.5 diagonals)")
        ap.add_argument("--spacing", type=float, nargs="+", default=[1.0], help="node spacing: one value or D H W")
        ap.add_argument("--step", type=float, default=None, help="sample distance (default: half the smallest spacing)")
        ap.add_argument("--opacity", type=float, default=None, help="scale of the table's A (default: 8 / the diagonal)")
        ap.add_argument("--t-min", type=float, default=0.0, help="end a ray once its transmittance is below this")
        ap.add_argument("--chunk", type=int, default=4, help="frames uploaded at a time and handed to one launch")
        ap.add_argument("--no-bricks", action="store_true", help="visit every sample: no jumps over empty bricks")
    else:
        ap.add_argument("--flows", default=None, metavar="FLOWS.npy", help="a [K,2,H,W] .npy: write its flow2rgb pictures")
        ap.add_argument("--flow-base", type=float, default=0.0, help="flow2rgb's background: 0 black, 1 white")
    ap.set_defaults(nd=nd)
    return ap


def series_source(args, nd):
    """(memory-mapped array, frame j -> its [*sp] block) of --seq or --field."""
    if (args.seq is None) == (args.field is None) and not (nd == 2 and args.flows and not args.seq and not args.field):
        raise SystemExit("exactly one of --seq and --field is needed")
    path = args.seq or args.field
    if path is None:
        return None, None, None
    a = np.load(path, mmap_mode="r")
    if args.field and a.ndim == nd + 2:
        if not 0 <= args.plane < a.shape[1]:
            raise SystemExit("--plane must lie in 0..%d" % (a.shape[1] - 1))
        take = lambda j0, j1: a[j0:j1, args.plane]
    elif a.ndim == nd + 1:
        take = lambda j0, j1: a[j0:j1]
    else:
        raise SystemExit("%s must be [K,%s]%s, got %s" % (path, ",".join("DHW"[3 - nd:]),
                                                        " or [K,NP,...]" if args.field else "", a.shape))
    return a, take, os.path.basename(path)


def _value_range(args, take, K):
    if args.range is not None:
        lo, hi = args.range
    else:
        lo, hi = float("inf"), float("-inf")
        for j in range(K):
            x = np.asarray(take(j, j + 1), np.float32)
            x = x[np.isfinite(x)]
            if x.size:
                lo, hi = min(lo, float(x.min())), max(hi, float(x.max()))
        if not lo <= hi:
            lo, hi = 0.0, 1.0
        if lo == hi:
            hi = lo + 1.0
    if not (-float("inf") < lo < hi < float("inf")):
        raise SystemExit("--range needs lo < hi, both finite")
    return float(lo), float(hi)


def _write(args, doc, images, pics=None):
    """--png-dir gets frame_%04d.png of `images` and flow_%04d.png of `pics`, --out the images and, beside it as
    <out>_flows.npy, the flow pictures, --json the report."""
    if args.png_dir:
        os.makedirs(args.png_dir, exist_ok=True)
        for stem, stack in (("frame", images), ("flow", pics)):
            for j, img in enumerate(stack if stack is not None else []):
                write_png(os.path.join(args.png_dir, "%s_%04d.png" % (stem, j)), to_uint8(img))
    arrays = {}
    if args.out and images is not None:
        arrays[args.out] = images
    if args.out and pics is not None:
        arrays[os.path.splitext(args.out)[0] + "_flows.npy"] = pics
    write_report(doc, args.json, arrays)


def main3d(argv=None):
    """flow3d: ray-cast a series of volumes."""
    args = _args(3, "Ray-cast a series of volumes or of 3-D fields to pictures").parse_args(argv)
    if args.chunk < 1 or min(args.image) < 1:
        raise SystemExit("--chunk and --image must be >= 1")
    if len(args.spacing) not in (1, 3) or not all(0 < h < float("inf") for h in args.spacing):
        raise SystemExit("--spacing takes one or 3 finite positive values")
    a, take, name = series_source(args, 3)
    K = int(a.shape[0])
    sp = tuple(int(s) for s in take(0, 1).shape[1:])
    spacing = args.spacing[0] if len(args.spacing) == 1 else tuple(args.spacing)
    lo, hi = _value_range(args, take, K)
    diag = float(np.linalg.norm(_extent(sp, spacing)))
    opacity = 8.0 / diag if args.opacity is None else args.opacity
    try:
        tf = load_tf(args.tf, args.tf_size, lo, hi, opacity)
        cams = np.stack([orbit_camera(sp, spacing, args.azimuth + j * args.orbit, args.elevation, args.distance, args.image,
                                      args.fov) for j in range(K)])
    except ValueError as e:
        raise SystemExit(str(e))
    dev = torch.device("cuda")
    source = lambda j0, j1: torch.from_numpy(np.array(take(j0, j1), np.float32)).to(dev)
    res = render_series(source, K, sp, cams, tf, lo, hi, args.image, args.step, spacing, args.mode, args.t_min, args.chunk,
                        not args.no_bricks, [j * args.dt for j in range(K)], keep_images=bool(args.out or args.png_dir))
    doc = {"source": name, "shape": list(sp), "plane": args.plane if args.field and a.ndim == 5 else None, "tf": args.tf,
           "range": [lo, hi], "opacity": opacity, "mode": args.mode, "image": list(args.image), "azimuth": args.azimuth,
           "elevation": args.elevation, "orbit": args.orbit, "fov": args.fov, "spacing": list(args.spacing),
           "step": args.step, "bricks": not args.no_bricks, "frames": res["frames"], "time_load_s": res["time_load_s"],
           "time_kernel_s": res["time_kernel_s"]}
    for w in res["frames"]:
        print("%s frame %d t %.4g: mean opacity %.4f  samples %d" % (name, w["frame"], w["time"], w["mean_opacity"], w["samples"]))
    print("load %.3f s  kernel %.4f s" % (res["time_load_s"], res["time_kernel_s"]))
    _write(args, doc, res["images"].numpy() if "images" in res else None)
    return doc


def main2d(argv=None, desc="Colour-map a series of 2-D frames or fields; flow2rgb pictures of flows"):
    """flow2d / upflow: 2-D frames or fields through the transfer function in torch (no kernel), flows through flow2rgb."""
    args = _args(2, desc).parse_args(argv)
    a, take, name = series_source(args, 2)
    dev = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    doc = {"source": name, "tf": args.tf, "frames": [], "flows": None}
    images = None
    if a is not None:
        K = int(a.shape[0])
        lo, hi = _value_range(args, take, K)
        try:
            tf = load_tf(args.tf, args.tf_size, lo, hi, 1.0)
        except ValueError as e:
            raise SystemExit(str(e))
        images = np.empty((K,) + tuple(take(0, 1).shape[1:]) + (4,), np.float32)
        for j in range(K):
            v = torch.from_numpy(np.array(take(j, j + 1), np.float32)).to(dev)
            img = colormap(v[0], tf, lo, hi)
            images[j] = img.cpu().numpy()
            doc["frames"].append({"frame": j, "time": j * args.dt, "mean_opacity": float(img[..., 3].mean()), "samples": 0})
        doc.update(shape=list(images.shape[1:3]), range=[lo, hi])
    pics = None
    if args.flows:
        fl = np.load(args.flows, mmap_mode="r")
        if fl.ndim != 4 or fl.shape[1] != 2:
            raise SystemExit("--flows must be [K,2,H,W], got %s" % (fl.shape,))
        pics = np.stack([flow2rgb(np.moveaxis(np.asarray(f, np.float32), 0, -1), args.flow_base) for f in fl])
        doc["flows"] = {"source": os.path.basename(args.flows), "count": int(fl.shape[0]), "base": args.flow_base}
    _write(args, doc, images, pics)
    print("%s: %d frames, %s flow pictures" % (name or args.flows, len(doc["frames"]), doc["flows"]["count"] if doc["flows"] else 0))
    return doc
