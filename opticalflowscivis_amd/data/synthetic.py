"""Seeded synthetic stand-ins for the reference's datasets.  There is no network and
the reference's pickles are not in the tree, so every benchmark / test input is generated here.
All generators are deterministic in (seed, shape) and produce float32 in [0, 1].
"""
import math

import torch


def _gen(seed, device):
    g = torch.Generator(device="cpu")
    g.manual_seed(int(seed))
    return g


def droplet3d_batch(B, S, seed=1234, device="cpu", radius=(40, 80), max_shift=4.0):
    """Droplet-3D-like triplets [B,3,S,S,S]: a binary {0,1} sphere (Droplet-3D is 0/255 bytes,
    README.md:24) translating by <= max_shift voxels per frame; radius range is given for S=256 and
    scales with S.  Channels = (frame t, frame t+2, frame t+1): (img0, img1, gt) as
    Flow-3D/train.py:150-151 slices them."""
    g = _gen(seed, device)
    scale = S / 256.0
    r = (torch.rand(B, generator=g) * (radius[1] - radius[0]) + radius[0]) * scale
    c0 = torch.rand(B, 3, generator=g) * (S - 2 * r.max() - 4 * max_shift) + r.max() + 2 * max_shift
    v = (torch.rand(B, 3, generator=g) * 2 - 1) * max_shift
    ax = torch.arange(S, dtype=torch.float32, device=device)
    out = torch.empty(B, 3, S, S, S, dtype=torch.float32, device=device)
    for b in range(B):
        for slot, t in ((0, 0.0), (1, 2.0), (2, 1.0)):
            c = (c0[b] + v[b] * t).to(device)
            d2 = ((ax - c[0]) ** 2).view(S, 1, 1) + ((ax - c[1]) ** 2).view(1, S, 1) + \
                 ((ax - c[2]) ** 2).view(1, 1, S)
            out[b, slot] = (d2 <= float(r[b]) ** 2).float()
    return out


def jets3d_batch(B, S, seed=1234, device="cpu", njets=5, max_shift=4.0):
    """5Jets-like smooth density triplets [B,3,S,S,S]: a sum of `njets` anisotropic Gaussian
    plumes advected by <= max_shift voxels per frame, min-max normalised to [0,1]."""
    g = _gen(seed, device)
    ax = torch.linspace(0, 1, S, device=device)
    out = torch.empty(B, 3, S, S, S, dtype=torch.float32, device=device)
    for b in range(B):
        cen = torch.rand(njets, 3, generator=g) * 0.6 + 0.2
        sig = torch.rand(njets, 3, generator=g) * 0.08 + 0.04
        vel = (torch.rand(njets, 3, generator=g) * 2 - 1) * max_shift / S
        for slot, t in ((0, 0.0), (1, 2.0), (2, 1.0)):
            vol = torch.zeros(S, S, S, device=device)
            for j in range(njets):
                c = cen[j] + vel[j] * t
                e = ((ax - float(c[0])) / float(sig[j, 0])).pow(2).view(S, 1, 1) + \
                    ((ax - float(c[1])) / float(sig[j, 1])).pow(2).view(1, S, 1) + \
                    ((ax - float(c[2])) / float(sig[j, 2])).pow(2).view(1, 1, S)
                vol += torch.exp(-0.5 * e)
            out[b, slot] = vol
        lo, hi = out[b].min(), out[b].max()
        out[b] = (out[b] - lo) / (hi - lo + 1e-12)
    return out


def droplet2d_batch(B, H=160, W=224, seed=1234, device="cpu", radius=(20, 40), max_shift=4.0):
    """Droplet-2D-like triplets [B,3,H,W]: a disc translating <= max_shift px/frame, blurred with a
    sigma=1 Gaussian; channels (t, t+2, t+1)."""
    g = _gen(seed, device)
    r = torch.rand(B, generator=g) * (radius[1] - radius[0]) + radius[0]
    cy = torch.rand(B, generator=g) * (H - 2 * radius[1] - 4 * max_shift) + radius[1] + 2 * max_shift
    cx = torch.rand(B, generator=g) * (W - 2 * radius[1] - 4 * max_shift) + radius[1] + 2 * max_shift
    v = (torch.rand(B, 2, generator=g) * 2 - 1) * max_shift
    ys = torch.arange(H, dtype=torch.float32, device=device).view(H, 1)
    xs = torch.arange(W, dtype=torch.float32, device=device).view(1, W)
    k = torch.exp(-0.5 * (torch.arange(-3, 4, dtype=torch.float32, device=device)) ** 2)
    k = (k / k.sum())
    out = torch.empty(B, 3, H, W, dtype=torch.float32, device=device)
    for b in range(B):
        for slot, t in ((0, 0.0), (1, 2.0), (2, 1.0)):
            d2 = (ys - float(cy[b] + v[b, 1] * t)) ** 2 + (xs - float(cx[b] + v[b, 0] * t)) ** 2
            out[b, slot] = (d2 <= float(r[b]) ** 2).float()
    flat = out.view(B * 3, 1, H, W)
    flat = torch.nn.functional.conv2d(torch.nn.functional.pad(flat, (3, 3, 0, 0), mode="replicate"),
                                      k.view(1, 1, 1, 7))
    flat = torch.nn.functional.conv2d(torch.nn.functional.pad(flat, (0, 0, 3, 3), mode="replicate"),
                                      k.view(1, 1, 7, 1))
    return flat.view(B, 3, H, W).clamp(0, 1)


def vortex2d_pairs(B, H=150, W=450, seed=0, device="cpu", nvort=8, max_shift=3.0):
    """Cylinder-ensemble-like pairs for UPFlow [B,2,3,H,W]: a sum of `nvort` Gaussian vortices
    advected between the two frames, min-max normalised, grey replicated to 3 channels
    (UPFlow/model/upflow.py:384-386)."""
    g = _gen(seed, device)
    ys = torch.arange(H, dtype=torch.float32, device=device).view(H, 1)
    xs = torch.arange(W, dtype=torch.float32, device=device).view(1, W)
    out = torch.empty(B, 2, 3, H, W, dtype=torch.float32, device=device)
    for b in range(B):
        cx = torch.rand(nvort, generator=g) * W
        cy = torch.rand(nvort, generator=g) * H
        sg = torch.rand(nvort, generator=g) * 18 + 8
        am = torch.rand(nvort, generator=g) * 2 - 1
        vx = torch.rand(nvort, generator=g) * max_shift
        vy = (torch.rand(nvort, generator=g) * 2 - 1) * 0.5 * max_shift
        for t in (0, 1):
            f = torch.zeros(H, W, device=device)
            for j in range(nvort):
                d2 = (xs - float(cx[j] + vx[j] * t)) ** 2 + (ys - float(cy[j] + vy[j] * t)) ** 2
                f += float(am[j]) * torch.exp(-0.5 * d2 / float(sg[j]) ** 2)
            out[b, t] = f
        lo, hi = out[b].min(), out[b].max()
        out[b] = (out[b] - lo) / (hi - lo + 1e-12)
    return out


# ---- whole sequences (sequence evaluation, opticalflowscivis_amd.evaluate): the motion models of the triplet generators
# above evaluated at t = 0 .. T-1.  The triplet generators stay as they are (fixtures and pins depend on their draws).

def _seq_start(g, T, S, r, v):
    """Start centre per axis so that the whole trajectory c0 + v t, t in [0, T-1], keeps the object inside [0, S)."""
    lo = r + 1 + torch.clamp(-v * (T - 1), min=0)
    hi = S - 1 - r - torch.clamp(v * (T - 1), min=0)
    u = torch.rand(v.shape, generator=g)
    return torch.where(hi > lo, lo + u * (hi - lo), (lo + hi) / 2)


def droplet3d_sequence(T, S, seed=1234, device="cpu", radius=(40, 80), max_shift=1.0):
    """[T,S,S,S]: the binary sphere of droplet3d_batch translating by <= max_shift voxels per frame, frames t = 0..T-1
    (radius range given for S=256, scaled with S)."""
    g = _gen(seed, device)
    r = float(torch.rand(1, generator=g) * (radius[1] - radius[0]) + radius[0]) * S / 256.0
    v = (torch.rand(3, generator=g) * 2 - 1) * max_shift
    c0 = _seq_start(g, T, S, r, v)
    ax = torch.arange(S, dtype=torch.float32, device=device)
    out = torch.empty(T, S, S, S, dtype=torch.float32, device=device)
    for t in range(T):
        c = (c0 + v * t).to(device)
        d2 = ((ax - c[0]) ** 2).view(S, 1, 1) + ((ax - c[1]) ** 2).view(1, S, 1) + ((ax - c[2]) ** 2).view(1, 1, S)
        out[t] = (d2 <= r * r).float()
    return out


def jets3d_sequence(T, S, seed=1234, device="cpu", njets=5, max_shift=1.0):
    """[T,S,S,S]: the Gaussian plumes of jets3d_batch advected by <= max_shift voxels per frame, frames t = 0..T-1,
    min-max normalised to [0,1] over the whole sequence."""
    g = _gen(seed, device)
    ax = torch.linspace(0, 1, S, device=device)
    cen = torch.rand(njets, 3, generator=g) * 0.6 + 0.2
    sig = torch.rand(njets, 3, generator=g) * 0.08 + 0.04
    vel = (torch.rand(njets, 3, generator=g) * 2 - 1) * max_shift / S
    out = torch.zeros(T, S, S, S, dtype=torch.float32, device=device)
    for t in range(T):
        for j in range(njets):
            c = cen[j] + vel[j] * t
            e = ((ax - float(c[0])) / float(sig[j, 0])).pow(2).view(S, 1, 1) + \
                ((ax - float(c[1])) / float(sig[j, 1])).pow(2).view(1, S, 1) + \
                ((ax - float(c[2])) / float(sig[j, 2])).pow(2).view(1, 1, S)
            out[t] += torch.exp(-0.5 * e)
    lo, hi = out.min(), out.max()
    return (out - lo) / (hi - lo + 1e-12)


def droplet2d_sequence(T, H=160, W=224, seed=1234, device="cpu", radius=(20, 40), max_shift=2.0):
    """[T,H,W]: the blurred disc of droplet2d_batch translating by <= max_shift px per frame, frames t = 0..T-1."""
    g = _gen(seed, device)
    r = float(torch.rand(1, generator=g) * (radius[1] - radius[0]) + radius[0])
    v = (torch.rand(2, generator=g) * 2 - 1) * max_shift  # (vy, vx)
    c0 = _seq_start(g, T, torch.tensor([float(H), float(W)]), r, v)
    ys = torch.arange(H, dtype=torch.float32, device=device).view(H, 1)
    xs = torch.arange(W, dtype=torch.float32, device=device).view(1, W)
    k = torch.exp(-0.5 * (torch.arange(-3, 4, dtype=torch.float32, device=device)) ** 2)
    k = k / k.sum()
    out = torch.empty(T, 1, H, W, dtype=torch.float32, device=device)
    for t in range(T):
        d2 = (ys - float(c0[0] + v[0] * t)) ** 2 + (xs - float(c0[1] + v[1] * t)) ** 2
        out[t, 0] = (d2 <= r * r).float()
    out = torch.nn.functional.conv2d(torch.nn.functional.pad(out, (3, 3, 0, 0), mode="replicate"), k.view(1, 1, 1, 7))
    out = torch.nn.functional.conv2d(torch.nn.functional.pad(out, (0, 0, 3, 3), mode="replicate"), k.view(1, 1, 7, 1))
    return out.view(T, H, W).clamp(0, 1)

def psnr(pred, gt):
    """PSNR on [0,1] data: -10 log10(mean((pred-gt)^2)) (Flow-3D/train.py:385)."""
    mse = torch.mean((pred.double() - gt.double()) ** 2)
    return float(-10.0 * math.log10(max(float(mse), 1e-20)))


def rectangle2d_sequence(n_frames=64, seed=1234, grid=(128, 128), box=(60, 80), tile=10, vel=(-6, 6),
                         max_seq=15):
    """Seeded restatement of Datasets/create_rectangle_2d.py:81-199 (BASELINE config C1): a box of
    `tile`-sized patches with values randint(30,256)/255 bouncing on a `grid`; the velocity is
    re-drawn every `max_seq` steps or when a wall is hit.  Keeps the original's axis swap
    (pos_x += vel_y, pos_y += vel_x, :165-167).  The original is unseeded and blocks on input();
    here numpy's and random's streams are replaced by one seeded numpy Generator.
    Returns (frames [T,H,W] float32 in [0,1], vel_x [T,H,W], vel_y [T,H,W])."""
    import numpy as np
    rng = np.random.default_rng(seed)
    gx, gy = grid
    bx, by = box
    b = np.ones((bx, by), dtype=np.float32)
    for i in range(0, bx, tile):
        for j in range(0, by, tile):
            b[i:i + tile, j:j + tile] = rng.integers(30, 256) / 255.0
    frames = np.zeros((n_frames, gx, gy), dtype=np.float32)
    vxs = np.zeros_like(frames)
    vys = np.zeros_like(frames)
    px, py = int(rng.integers(0, gx - bx + 1)), int(rng.integers(0, gy - by + 1))
    vx, vy = int(rng.integers(vel[0], vel[1] + 1)), int(rng.integers(vel[0], vel[1] + 1))
    seq = max_seq
    for t in range(n_frames):
        if seq == 0:
            vx, vy = int(rng.integers(vel[0], vel[1] + 1)), int(rng.integers(vel[0], vel[1] + 1))
            seq = max_seq
        px = min(max(px + vy, 0), gx - bx)
        py = min(max(py + vx, 0), gy - by)
        frames[t, px:px + bx, py:py + by] = b
        vxs[t, px:px + bx, py:py + by] = vx
        vys[t, px:px + bx, py:py + by] = vy
        seq -= 1
        if px == 0 or py == 0 or px == gx - bx or py == gy - by:
            seq = 0
    return torch.from_numpy(frames), torch.from_numpy(vxs), torch.from_numpy(vys)


def rectangle2d_triplet(t=0, seed=1234):
    """(img0, img1, gt) = frames (t, t+2, t+1) as [1,3,128,128] (C1: pair + middle frame)."""
    f, _, _ = rectangle2d_sequence(t + 3, seed)
    return torch.stack([f[t], f[t + 2], f[t + 1]], 0).unsqueeze(0)


# ---- ground-truth motion (flow evaluation, opticalflowscivis_amd.flow_eval): each *_motion generator returns the frames
# of its *_sequence counterpart, bit for bit (the same draws in the same order), and gt(t_from, t_to) -> (disp, valid,
# noc): the displacement from frame t_from to frame t_to at the pixels of frame t_from, [2,H,W] (x along W, y along H)
# or [3,D,H,W] (x, y, z along D), in elements, fp32 on the frames' device, with bool masks [*spatial].  Warping frame
# t_to with disp (out(p) = frame_t_to(p + disp(p)), the RIFE / PWC warps) gives frame t_from where noc is set.  noc is a
# subset of valid; occluded = valid and not noc: pixels that are covered by the object in frame t_to without being part
# of it in frame t_from, and pixels whose target p + disp leaves the grid.

def _occlusion(disp, inside_to, moving_from):
    """Occluded pixels of frame t_from: background (not `moving_from`) covered by the object in frame t_to, or a target
    p + disp outside the grid."""
    nd = disp.shape[0]
    sp = disp.shape[1:]
    out = torch.zeros(sp, dtype=torch.bool, device=disp.device)
    for c in range(nd):  # channel c moves along spatial axis nd - 1 - c
        n = sp[nd - 1 - c]
        ax = torch.arange(n, dtype=disp.dtype, device=disp.device).view([-1 if a == nd - 1 - c else 1
                                                                          for a in range(nd)])
        tgt = ax + disp[c]
        out |= (tgt < 0) | (tgt > n - 1)
    return out | (inside_to & ~moving_from)


def rectangle2d_motion(n_frames=64, seed=1234, grid=(128, 128), box=(60, 80), tile=10, vel=(-6, 6), max_seq=15):
    """(frames [T,H,W], gt) for rectangle2d_sequence.  The box's displacement comes from its actual positions, found
    in the frames (every box pixel is >= 30/255, the background 0): at a wall `pos += vel` is clamped, so the stored
    velocity is wrong there.  The generator swaps axes (rows move by vel_y), so channel 0 (along W) is the column
    shift.  The background does not move; every pixel is valid."""
    frames, _, _ = rectangle2d_sequence(n_frames, seed, grid, box, tile, vel, max_seq)
    H, W = frames.shape[1:]
    bx, by = box
    rows = (frames > 0).any(2)
    cols = (frames > 0).any(1)
    px = [int(torch.nonzero(rows[t])[0]) if rows[t].any() else 0 for t in range(frames.shape[0])]
    py = [int(torch.nonzero(cols[t])[0]) if cols[t].any() else 0 for t in range(frames.shape[0])]

    def box_mask(t):
        m = torch.zeros(H, W, dtype=torch.bool, device=frames.device)
        m[px[t]:px[t] + bx, py[t]:py[t] + by] = True
        return m

    def gt(t_from, t_to):
        inside = box_mask(t_from)
        disp = torch.zeros(2, H, W, dtype=torch.float32, device=frames.device)
        disp[0][inside] = float(py[t_to] - py[t_from])
        disp[1][inside] = float(px[t_to] - px[t_from])
        valid = torch.ones(H, W, dtype=torch.bool, device=frames.device)
        return disp, valid, ~_occlusion(disp, box_mask(t_to), inside)

    return frames, gt


def droplet2d_motion(T, H=160, W=224, seed=1234, device="cpu", radius=(20, 40), max_shift=2.0, v=None):
    """(frames [T,H,W], gt) for droplet2d_sequence: the disc moves by (vy, vx) per frame, so the displacement is
    (vx, vy) dt inside the disc of frame t_from and 0 outside; `valid` leaves out a 3-px band (the blur's support)
    around the disc's boundary.  v = (vy, vx) replaces the drawn velocity (the draws stay the same; the frames then
    differ from droplet2d_sequence's)."""
    g = _gen(seed, device)
    r = float(torch.rand(1, generator=g) * (radius[1] - radius[0]) + radius[0])
    vd = (torch.rand(2, generator=g) * 2 - 1) * max_shift  # (vy, vx)
    if v is not None:
        vd = torch.tensor([float(v[0]), float(v[1])])
    v = vd
    c0 = _seq_start(g, T, torch.tensor([float(H), float(W)]), r, v)
    ys = torch.arange(H, dtype=torch.float32, device=device).view(H, 1)
    xs = torch.arange(W, dtype=torch.float32, device=device).view(1, W)
    k = torch.exp(-0.5 * (torch.arange(-3, 4, dtype=torch.float32, device=device)) ** 2)
    k = k / k.sum()
    out = torch.empty(T, 1, H, W, dtype=torch.float32, device=device)
    for t in range(T):
        d2 = (ys - float(c0[0] + v[0] * t)) ** 2 + (xs - float(c0[1] + v[1] * t)) ** 2
        out[t, 0] = (d2 <= r * r).float()
    out = torch.nn.functional.conv2d(torch.nn.functional.pad(out, (3, 3, 0, 0), mode="replicate"), k.view(1, 1, 1, 7))
    out = torch.nn.functional.conv2d(torch.nn.functional.pad(out, (0, 0, 3, 3), mode="replicate"), k.view(1, 1, 7, 1))
    frames = out.view(T, H, W).clamp(0, 1)

    def dist(t):
        return torch.sqrt((ys - float(c0[0] + v[0] * t)) ** 2 + (xs - float(c0[1] + v[1] * t)) ** 2)

    def gt(t_from, t_to):
        dt = float(t_to - t_from)
        d0 = dist(t_from)
        inside = d0 <= r
        disp = torch.zeros(2, H, W, dtype=torch.float32, device=device)
        disp[0][inside] = float(v[1]) * dt
        disp[1][inside] = float(v[0]) * dt
        valid = (d0 - r).abs() > 3
        return disp, valid, valid & ~_occlusion(disp, dist(t_to) <= r, inside)

    return frames, gt


def droplet3d_motion(T, S, seed=1234, device="cpu", radius=(40, 80), max_shift=1.0, v=None):
    """(frames [T,S,S,S], gt) for droplet3d_sequence: the centre is indexed (D, H, W), so the displacement is
    (v[2], v[1], v[0]) dt as (x, y, z) inside the sphere of frame t_from, 0 outside; `valid` leaves out a 1-voxel band
    around the sphere's boundary.  v (along D, H, W) replaces the drawn velocity as in droplet2d_motion."""
    g = _gen(seed, device)
    r = float(torch.rand(1, generator=g) * (radius[1] - radius[0]) + radius[0]) * S / 256.0
    vd = (torch.rand(3, generator=g) * 2 - 1) * max_shift
    if v is not None:
        vd = torch.tensor([float(a) for a in v])
    v = vd
    c0 = _seq_start(g, T, S, r, v)
    ax = torch.arange(S, dtype=torch.float32, device=device)
    frames = torch.empty(T, S, S, S, dtype=torch.float32, device=device)

    def d2(t):
        c = (c0 + v * t).to(device)
        return ((ax - c[0]) ** 2).view(S, 1, 1) + ((ax - c[1]) ** 2).view(1, S, 1) + ((ax - c[2]) ** 2).view(1, 1, S)

    for t in range(T):
        frames[t] = (d2(t) <= r * r).float()

    def gt(t_from, t_to):
        dt = float(t_to - t_from)
        q = d2(t_from)
        inside = q <= r * r
        disp = torch.zeros(3, S, S, S, dtype=torch.float32, device=device)
        for c in range(3):
            disp[c][inside] = float(v[2 - c]) * dt
        valid = (torch.sqrt(q) - r).abs() > 1
        return disp, valid, valid & ~_occlusion(disp, d2(t_to) <= r * r, inside)

    return frames, gt


def jets3d_motion(T, S, seed=1234, device="cpu", njets=5, max_shift=1.0):
    """(frames [T,S,S,S], gt) for jets3d_sequence.  Plume j moves by vel_j per frame on axes linspace(0, 1, S) indexed
    (D, H, W): (vel_j[2], vel_j[1], vel_j[0]) (S-1) voxels as (x, y, z).  The ground truth is the density-weighted mean
    over the plumes, sum_j rho_j v_j / sum_j rho_j (rho_j unnormalised, at frame t_from); valid where the normalised
    density of frame t_from exceeds 0.05; no occlusion (noc = valid)."""
    g = _gen(seed, device)
    ax = torch.linspace(0, 1, S, device=device)
    cen = torch.rand(njets, 3, generator=g) * 0.6 + 0.2
    sig = torch.rand(njets, 3, generator=g) * 0.08 + 0.04
    vel = (torch.rand(njets, 3, generator=g) * 2 - 1) * max_shift / S

    def plume(j, t):
        c = cen[j] + vel[j] * t
        e = ((ax - float(c[0])) / float(sig[j, 0])).pow(2).view(S, 1, 1) + \
            ((ax - float(c[1])) / float(sig[j, 1])).pow(2).view(1, S, 1) + \
            ((ax - float(c[2])) / float(sig[j, 2])).pow(2).view(1, 1, S)
        return torch.exp(-0.5 * e)

    out = torch.zeros(T, S, S, S, dtype=torch.float32, device=device)
    for t in range(T):
        for j in range(njets):
            out[t] += plume(j, t)
    lo, hi = out.min(), out.max()
    frames = (out - lo) / (hi - lo + 1e-12)

    def gt(t_from, t_to):
        dt = float(t_to - t_from)
        num = torch.zeros(3, S, S, S, dtype=torch.float64, device=device)
        den = torch.zeros(S, S, S, dtype=torch.float64, device=device)
        for j in range(njets):
            rho = plume(j, t_from).double()
            den += rho
            for c in range(3):
                num[c] += rho * (float(vel[j, 2 - c]) * (S - 1) * dt)
        disp = torch.where(den > 0, num / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(num))
        valid = frames[t_from] > 0.05
        return disp.float(), valid, valid.clone()

    return frames, gt
