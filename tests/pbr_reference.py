"""Float64 restatement of the image-based-lighting stage: the nvdiffrast.torch.texture calls of pbr/light.py and pbr/shade.py
(cube maps with bilinear filtering across face edges, the 2-D clamp lookup of the BRDF LUT, trilinear mip selection by
mip_level_bias), the renderutils diffuse / specular cube convolutions, CubemapLight.build_mips with its own mip backward, and
the pbr_shading composition.  CPU torch in float64; autograd supplies every gradient except the mip backward (the reference's
own, restated as a custom Function).  The sampling rules are those of csrc/pbr.hip (DESIGN.md "PBR stage"): the face is the
largest |component| (z only when strictly largest, then y only when strictly larger than x); a bilinear tap off one face edge
is the neighbouring face's texel that holds the tap's texel-centre direction; a corner tap gives its weight in thirds to the
other three taps; a zero direction samples 0."""
import numpy as np
import torch

MIN_ROUGHNESS, MAX_ROUGHNESS, LIGHT_MIN_RES = 0.08, 0.5, 8


# ---- cube geometry (numpy; integer or float arrays) ------------------------------------------------------------------------
def _cube_dir(f, a, b, m):
    """Direction (scaled by m) of face-local (a, b) on face f (pbr/light.py cube_to_dir)."""
    one = np.ones_like(a) * m
    x = np.select([f == 0, f == 1, f == 2, f == 3, f == 4], [one, -one, a, a, a], -a)
    y = np.select([f == 0, f == 1, f == 2, f == 3, f == 4], [-b, -b, one, -one, -b], -b)
    z = np.select([f == 0, f == 1, f == 2, f == 3, f == 4], [-a, a, b, -b, one], -one)
    return x, y, z


def _face_of(x, y, z):
    ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
    return np.where(az > np.maximum(ax, ay), np.where(z < 0, 5, 4),
                    np.where(ay > ax, np.where(y < 0, 3, 2), np.where(x < 0, 1, 0)))


def _face_coords(f, x, y, z):
    """(a, b, m): face-local coordinates and major magnitude of (x, y, z) on face f."""
    m = np.select([f == 0, f == 1, f == 2, f == 3, f == 4], [x, -x, y, -y, z], -z)
    a = np.select([f == 0, f == 1, f == 2, f == 3, f == 4], [-z, z, x, x, x], -x)
    b = np.select([f == 0, f == 1, f == 2, f == 3, f == 4], [-y, -y, z, -z, -y], -y)
    return a, b, m


def _cube_tap(f, x, y, N):
    """Texel index of tap (x, y) on face f; -2 for a corner tap; a tap off one edge wraps onto the neighbouring face."""
    ox, oy = (x < 0) | (x >= N), (y < 0) | (y >= N)
    inside = (f * N + y) * N + x
    dx, dy, dz = _cube_dir(f, 2 * x + 1 - N, 2 * y + 1 - N, N)
    g = _face_of(dx, dy, dz)
    a, b, m = _face_coords(g, dx, dy, dz)
    m = np.maximum(m, 1)
    nx = np.clip((a + m) * N // (2 * m), 0, N - 1)
    ny = np.clip((b + m) * N // (2 * m), 0, N - 1)
    wrapped = (g * N + ny) * N + nx
    return np.where(~ox & ~oy, inside, np.where(ox & oy, -2, wrapped))


def cube_taps(dirs, N):
    """dirs [n, 3] -> texel indices [n, 4] (-1: no texel) and bilinear weights [n, 4] (float64) on an N x N cube."""
    d = np.asarray(dirs, np.float64).reshape(-1, 3)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    f = _face_of(x, y, z)
    a, b, m = _face_coords(f, x, y, z)
    valid = (m > 0) & np.isfinite(a) & np.isfinite(b) & np.isfinite(m)
    ms = np.where(valid, m, 1.0)
    a, b = np.where(valid, a, 0.0), np.where(valid, b, 0.0)
    u = np.clip((a / ms + 1.0) * 0.5, 0.0, 1.0)
    v = np.clip((b / ms + 1.0) * 0.5, 0.0, 1.0)
    sx, sy = u * N - 0.5, v * N - 0.5
    x0, y0 = np.floor(sx), np.floor(sy)
    fx, fy = sx - x0, sy - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    w = np.stack([(1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy], 1)
    idx = np.stack([_cube_tap(f, x0, y0, N), _cube_tap(f, x0 + 1, y0, N), _cube_tap(f, x0, y0 + 1, N),
                    _cube_tap(f, x0 + 1, y0 + 1, N)], 1)
    corner = idx == -2
    share = (w * corner).sum(1, keepdims=True) / 3.0
    w = np.where(corner, 0.0, w + share * corner.any(1, keepdims=True))
    idx = np.where(corner, -1, idx)
    w[~valid] = 0.0
    idx[~valid] = -1
    return idx, w


def cube_sample(tex, dirs):
    """tex [6, N, N, C] (torch, any grad) at dirs [n, 3] (numpy or a tensor without grad) -> [n, C]."""
    if isinstance(dirs, torch.Tensor):
        if dirs.requires_grad:
            raise ValueError("cube lookups take no gradient with respect to the direction")
        dirs = dirs.detach().cpu().numpy()
    N, C = tex.shape[1], tex.shape[-1]
    idx, w = cube_taps(dirs, N)
    flat = tex.reshape(-1, C)
    wt = torch.from_numpy(w).to(tex.dtype)
    it = torch.from_numpy(np.maximum(idx, 0))
    return sum(wt[:, k:k + 1] * flat[it[:, k]] for k in range(4))


def flat_sample(tex, uv):
    """tex [H, W, C] at uv [n, 2] with the clamp boundary; differentiable with respect to tex and uv."""
    H, W, C = tex.shape
    sx = (uv[:, 0] * W - 0.5).clamp(-1.0, float(W))
    sy = (uv[:, 1] * H - 0.5).clamp(-1.0, float(H))
    x0, y0 = torch.floor(sx).detach(), torch.floor(sy).detach()
    fx, fy = (sx - x0)[:, None], (sy - y0)[:, None]
    xa, xb = x0.clamp(0, W - 1).long(), (x0 + 1).clamp(0, W - 1).long()
    ya, yb = y0.clamp(0, H - 1).long(), (y0 + 1).clamp(0, H - 1).long()
    return ((1 - fx) * (1 - fy) * tex[ya, xa] + fx * (1 - fy) * tex[ya, xb] + (1 - fx) * fy * tex[yb, xa]
            + fx * fy * tex[yb, xb])


def texture(tex, uv, filter_mode="auto", boundary_mode="wrap", mip=None, mip_level_bias=None):
    """nvdiffrast.torch.texture for the reference's three call shapes, float64: tex [1, 6, N, N, C] with boundary "cube" (uv =
    directions [1, h, w, 3]) or [1, H, W, C] with "clamp" (uv [1, h, w, 2]); filter "linear", or "linear-mipmap-linear" with an
    explicit mip list and mip_level_bias [1, h, w]."""
    cube = boundary_mode == "cube"
    lead = uv.shape[:-1]
    levels = [tex[0]] + ([m[0] for m in mip] if mip is not None else [])
    coords = uv.reshape(-1, uv.shape[-1])

    def one(t):
        return cube_sample(t, coords) if cube else flat_sample(t, coords)

    if filter_mode == "linear" or mip_level_bias is None or len(levels) == 1:
        out = one(levels[0])
    else:
        L = len(levels)
        lv = mip_level_bias.reshape(-1).clamp(0.0, float(L - 1))
        l0 = torch.floor(lv).detach().clamp(max=L - 1)
        l1 = (l0 + 1).clamp(max=L - 1)
        t = (lv - l0)[:, None]
        out = 0
        for li, lt in enumerate(levels):
            wl = (1 - t) * (l0 == li).to(t.dtype)[:, None] + t * (l1 == li).to(t.dtype)[:, None]
            out = out + wl * one(lt)
    return out.reshape(*lead, levels[0].shape[-1])


# ---- prefilter ------------------------------------------------------------------------------------------------------------
def texel_dirs(N):
    """Normalised texel-centre directions [6 N N, 3] and per-texel solid-angle weights [6 N N] (renderutils' atan form)."""
    f, y, x = np.meshgrid(np.arange(6), np.arange(N), np.arange(N), indexing="ij")
    f, y, x = f.ravel(), y.ravel(), x.ravel()
    fx = 2.0 * ((x + 0.5) / N) - 1.0
    fy = 2.0 * ((y + 0.5) / N) - 1.0
    d = np.stack(_cube_dir(f, fx, fy, 1.0), 1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    if N > 1:
        H = N // 2
        ax, ay = np.abs(x - H), np.abs(y - H)
        area = (np.arctan((ax + 1) / H) - np.arctan(ax / H)) * (np.arctan((ay + 1) / H) - np.arctan(ay / H))
    else:
        area = np.ones(6)
    return d, area


def _diffuse_rows(N, r0, r1):
    d, area = texel_dirs(N)
    c = np.clip(d[r0:r1] @ d.T, 0.0, 0.999)
    return c * area[None, :] / 3.141592


def ndf_cutoff(roughness, cutoff=0.99):
    """The cosine that keeps `cutoff` of the GGX lobe's energy (renderutils' host-side search, restated)."""
    def ndf(a2, c):
        c = np.clip(c, 0.0, 1.0)
        dd = (c * a2 - c) * c + 1.0
        return a2 / (dd * dd * np.pi)
    costheta = np.cos(np.linspace(0, np.pi / 2.0, 1000000))
    D = np.cumsum(ndf(roughness ** 4, costheta))
    return float(costheta[np.argmax(D >= D[..., -1] * cutoff)])


def _specular_rows(N, roughness, cut, r0, r1):
    d, area = texel_dirs(N)
    V, L = d[r0:r1, None, :], d[None, :, :]
    dot = (V * L).sum(-1)
    Hv = V + L
    hl = np.linalg.norm(Hv, axis=-1, keepdims=True)
    Hv = np.where(hl > 0, Hv / np.where(hl > 0, hl, 1.0), Hv)
    noh = np.clip((V * Hv).sum(-1), 0.0, 1.0)
    a2 = (roughness * roughness) ** 2
    dd = (noh * a2 - noh) * noh + 1.0
    D = a2 / (dd * dd * np.pi)
    return np.where(dot >= cut, np.maximum(dot, 0.0) * D * area[None, :] / 4.0, 0.0)


class _RowOp(torch.autograd.Function):
    """out = M @ x with M built in row chunks (never whole); backward M^T @ dout."""
    @staticmethod
    def forward(ctx, x, rows, T):
        ctx.rows, ctx.T = rows, T
        xf = x.reshape(T, -1)
        out = torch.cat([torch.from_numpy(rows(r, min(T, r + 512))) @ xf for r in range(0, T, 512)])
        return out.reshape(x.shape)

    @staticmethod
    def backward(ctx, g):
        T = ctx.T
        gf = g.reshape(T, -1)
        out = sum(torch.from_numpy(ctx.rows(r, min(T, r + 512))).T @ gf[r:min(T, r + 512)] for r in range(0, T, 512))
        return out.reshape(g.shape), None, None


def diffuse_cubemap(cube):
    N = cube.shape[1]
    return _RowOp.apply(cube, lambda r0, r1: _diffuse_rows(N, r0, r1), 6 * N * N)


_SPECULAR = {}


class _SparseOp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, M):
        ctx.M = M
        return torch.sparse.mm(M, x.reshape(M.shape[1], -1)).reshape(x.shape)

    @staticmethod
    def backward(ctx, g):
        return torch.sparse.mm(ctx.M.t(), g.reshape(ctx.M.shape[0], -1)).reshape(g.shape), None


def _specular_matrix(N, roughness, cut):
    """The (sparse: only texels inside the lobe's cutoff) weight matrix and its row sums, cached per (N, roughness, cutoff)."""
    key = (N, float(roughness), float(cut))
    if key not in _SPECULAR:
        T, rows, cols, vals = 6 * N * N, [], [], []
        for r in range(0, T, 512):
            m = _specular_rows(N, roughness, cut, r, min(T, r + 512))
            i, j = np.nonzero(m)
            rows.append(i + r)
            cols.append(j)
            vals.append(m[i, j])
        idx = torch.from_numpy(np.stack([np.concatenate(rows), np.concatenate(cols)]))
        M = torch.sparse_coo_tensor(idx, torch.from_numpy(np.concatenate(vals)), (T, T)).coalesce()
        wsum = torch.sparse.sum(M, 1).to_dense()
        _SPECULAR[key] = (M, wsum)
    return _SPECULAR[key]


def specular_cubemap(cube, roughness, cutoff=0.99):
    N = cube.shape[1]
    M, wsum = _specular_matrix(N, roughness, ndf_cutoff(roughness, cutoff))
    return _SparseOp.apply(cube, M) / wsum.to(cube.dtype).reshape(6, N, N, 1)


class CubemapMip(torch.autograd.Function):
    """2x2 average forward; the reference's backward: cube lookup of 0.25 dout at the finer level's texel-centre directions."""
    @staticmethod
    def forward(ctx, cube):
        return torch.nn.functional.avg_pool2d(cube.permute(0, 3, 1, 2), (2, 2)).permute(0, 2, 3, 1).contiguous()

    @staticmethod
    def backward(ctx, dout):
        res = dout.shape[1] * 2
        dirs, _ = texel_dirs(res)  # pbr/light.py:39-54: linspace texel centres, cube_to_dir, normalize
        return cube_sample(dout * 0.25, dirs).reshape(6, res, res, dout.shape[-1])


# ---- light and shading ----------------------------------------------------------------------------------------------------
class Light64:
    """CubemapLight in float64 on the CPU (same mip chain, roughness schedule and get_mip)."""
    def __init__(self, base):
        self.base = base

    def build_mips(self, cutoff=0.99):
        self.specular = [self.base]
        while self.specular[-1].shape[1] > LIGHT_MIN_RES:
            self.specular.append(CubemapMip.apply(self.specular[-1]))
        self.diffuse = diffuse_cubemap(self.specular[0])
        n = len(self.specular)
        for i in range(n - 1):
            r = (i / (n - 2)) * (MAX_ROUGHNESS - MIN_ROUGHNESS) + MIN_ROUGHNESS
            self.specular[i] = specular_cubemap(self.specular[i], r, cutoff)
        self.specular[-1] = specular_cubemap(self.specular[-1], 1.0, cutoff)

    def get_mip(self, roughness):
        n = len(self.specular)
        return torch.where(
            roughness < MAX_ROUGHNESS,
            (roughness.clamp(MIN_ROUGHNESS, MAX_ROUGHNESS) - MIN_ROUGHNESS) / (MAX_ROUGHNESS - MIN_ROUGHNESS) * (n - 2),
            (roughness.clamp(MAX_ROUGHNESS, 1.0) - MAX_ROUGHNESS) / (1.0 - MAX_ROUGHNESS) + n - 2)


def aces_film(x):
    return ((x * (2.51 * x + 0.03)) / (x * (2.43 * x + 0.59) + 0.14)).clamp(0.0, 1.0)


def linear_to_srgb(x):
    eps = torch.finfo(torch.float32).eps
    return torch.where(x <= 0.0031308, 323 / 25 * x, (211 * torch.clamp(x, min=eps) ** (5 / 12) - 11) / 200)


def pbr_shading(light, normals, view_dirs, albedo, roughness, mask, tone=False, gamma=False, occlusion=None, metallic=None,
                brdf_lut=None, background=None):
    """pbr_shading on [H, W, *] float64 tensors; returns the same keys ([H, W, 3] each)."""
    H, W, _ = normals.shape
    n = normals.reshape(-1, 3)
    v = view_dirs.reshape(-1, 3)
    nv = (n * v).sum(-1, keepdim=True)
    ref = 2.0 * nv.clamp(min=0.0) * n - v
    dpow = light.diffuse.pow(1.0 / 2.2).clamp(0.0, 1.0)
    dl = cube_sample(dpow, n.detach())
    if occlusion is not None:
        dl = dl * occlusion.reshape(-1, 1)
    alb = albedo.reshape(-1, 3)
    diffuse_rgb = dl * alb
    nov = nv.clamp(1e-4, 1.0)
    rough = roughness.reshape(-1, 1)
    fg = flat_sample(brdf_lut.reshape(brdf_lut.shape[-3:]), torch.cat([nov, rough], -1))
    lvl = light.get_mip(rough)[:, 0]
    spec = texture(light.specular[0][None], ref.detach()[None], "linear-mipmap-linear", "cube",
                   mip=[m[None] for m in light.specular[1:]], mip_level_bias=lvl)
    f0 = 0.04 * torch.ones_like(alb) if metallic is None else (1.0 - metallic.reshape(-1, 1)) * 0.04 + alb * metallic.reshape(-1, 1)
    specular_rgb = spec * (f0 * fg[:, 0:1])
    rgb = diffuse_rgb + specular_rgb
    rgb = aces_film(rgb) if tone else rgb.clamp(0.0, 1.0)
    if gamma:
        rgb = linear_to_srgb(rgb)
    bg = torch.zeros_like(rgb) if background is None else background.reshape(-1, 3)
    rgb = torch.where(mask.reshape(-1, 1) > 0, rgb, bg)
    shape = (H, W, 3)
    return {"render_rgb": rgb.reshape(shape), "diffuse_rgb": diffuse_rgb.reshape(shape),
            "specular_rgb": specular_rgb.reshape(shape), "diffuse_light": dl.reshape(shape)}


def envmap_dirs(res):
    """export_envmap's latitude-longitude directions [h, w, 3]."""
    gy, gx = np.meshgrid(np.linspace(0.0, 1.0, res[0]), np.linspace(-1.0, 1.0, res[1]), indexing="ij")
    st, ct = np.sin(gy * np.pi), np.cos(gy * np.pi)
    sp, cp = np.sin(gx * np.pi), np.cos(gx * np.pi)
    return np.stack((st * sp, ct, -st * cp), -1)


# ---- fixture inputs (tests/golden/make_golden_pbr.py and the tests rebuild them: only the outputs are stored) --------------------
def _u01(shape, salt):
    """Deterministic uniform [0, 1) values from a splitmix64 hash of the element index: bit-identical on every machine."""
    n = int(np.prod(shape))
    with np.errstate(over="ignore"):
        x = np.arange(n, dtype=np.uint64) + np.uint64(salt) * np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    return ((x >> np.uint64(11)).astype(np.float64) * 2.0 ** -53).reshape(shape)


def _f32(x):
    """Round to float32 values (what the kernels see), kept in float64."""
    return np.asarray(x, np.float32).astype(np.float64)


def fixture_inputs(H=17, W=23):
    """The inputs of tests/golden/pbr_light.npz: lights of base 32 and 16, H x W pixels (face edges, cube corners, roughness on
    get_mip's bounds and NoV at its clamp planted) and the weights of the summed losses.  All float32 values except the planted
    roughness (exactly 0.08 / 0.5 / 1.0, which float32 rounds off the bound for float64 arithmetic)."""
    out = {"base32": _f32((0.5 + 1.0 * _u01((6, 32, 32, 3), 1)) ** 2 * 0.5), "base16": _f32(0.1 + 0.9 * _u01((6, 16, 16, 3), 2))}
    n = 2.0 * _u01((H * W, 3), 3) - 1.0
    special = np.array([[1, 1, 0], [1, -1, 0], [0, 1, 1], [1, 0, -1], [1, 1, 1], [-1, 1, -1], [1, -1, -1], [0, 0, 1],
                        [0.3, 1, 1], [1, 0.999, 0.2]], np.float64)
    k = min(len(special), n.shape[0])
    n[:k] = special[:k]
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    v = n + 0.6 * (2.0 * _u01((H * W, 3), 4) - 1.0)
    v[5::9] = -n[5::9]  # back-facing: NoV at its clamp
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    rough = _f32(_u01((H * W, 1), 5))
    rough[:4, 0] = [0.08, 0.5, 1.0, 0.3][:H * W]
    px = dict(normals=_f32(n), view_dirs=_f32(v), albedo=_f32(0.05 + 0.9 * _u01((H * W, 3), 6)), roughness=rough,
              occlusion=_f32(0.3 + 0.7 * _u01((H * W, 1), 7)), metallic=_f32(_u01((H * W, 1), 8)),
              mask=(_u01((H * W, 1), 9) > 0.2).astype(np.float64))
    out.update({"px_" + key: val.reshape(H, W, -1) for key, val in px.items()})
    for i, key in enumerate(("render_rgb", "diffuse_rgb", "specular_rgb", "diffuse_light")):
        out["w_" + key] = _f32(2.0 * _u01((H, W, 3), 10 + i) - 1.0)
    for i, (key, shape) in enumerate((("mip", (6, 8, 8, 3)), ("diffuse", (6, 16, 16, 3)), ("specular", (6, 16, 16, 3)),
                                      ("envmap", (16, 32, 3)))):
        out["w16_" + key] = _f32(2.0 * _u01(shape, 20 + i) - 1.0)
    return out

