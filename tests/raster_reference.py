"""A float64 restatement of the reference rasterizer, independent of the CPU oracle and of the HIP kernels.

Written from the behaviour of the reference CUDA rasterizer (CR = submodules/diff-gaussian-rasterization/cuda_rasterizer,
citations file:line): dense over (pixel x Gaussian), torch float64 on the CPU, small scenes only.

  forward preprocess   CR/forward.cu:155-256 -- near-plane test z <= 0.2 (CR/auxiliary.h:154), projection with
                       p_w = 1 / (w + 1e-7) (CR/forward.cu:199), radius ceil(3 sqrt(lambda_max)) with the 0.1 floor
                       (CR/forward.cu:230-232), tile rect getRect (CR/auxiliary.h:46-56), ndc2pix (CR/auxiliary.h:41-44)
  3D covariance        CR/forward.cu:118-152 -- the quaternion is used as given, not normalised; the scale that enters is
                       scale_modifier * scale (CR/forward.cu:122-124), and the scale gradient is taken with respect to THAT
                       product (CR/backward.cu:295,323-325 carry no factor of the modifier): here the modified scale is the leaf
  EWA 2D covariance    CR/forward.cu:74-113 -- t.x / t.z, t.y / t.z clamped to +-1.3 tan(fov/2), J from the clamped t,
                       focal lengths W / (2 tan_fovx), H / (2 tan_fovy) (CR/rasterizer_impl.cu:224-225), +0.3 dilation
  SH -> RGB            CR/forward.cu:20-71 -- direction from campos, +0.5, clamped at 0
  blend                CR/forward.cu:261-383 -- front to back in depth order per tile; a pair is skipped when power > 0
                       (:341) or alpha = min(0.99, o G) < 1/255 (:348-349); the list ends before the Gaussian that would take
                       T below 1e-4 (:352); color = sum c alpha T + T_final bg, depth = sum z alpha T, alpha = sum alpha T

The discrete decisions (culling, radii, tile rects, depth order, the three blend thresholds) are taken under no_grad.  The
gradients come from autograd, so they do not share the hand-derived backward (CR/backward.cu).  Three places where
CR/backward.cu is deliberately not the exact gradient of the forward are emulated:

  1. the 0.99 alpha clamp passes the unclamped gradient, dL_dG = opacity * dL_dalpha (CR/backward.cu:566-567): here a
     straight-through min;
  2. under the frustum clamp t.x / t.y enter J as constants: x_grad_mul / y_grad_mul = 0 (CR/backward.cu:175-176,262-263)
     and dL_dtz is the partial with t.x, t.y held (:264): here where(inside, t.x, (lim t.z).detach());
  3. the depth image gives no gradient to the means, only to alpha (CR/backward.cu:541-549): here the blended view z is
     detached.

Not emulated: denom2inv's +1e-7 (CR/backward.cu:203).  det(cov2D) >= 0.09 because of the 0.3 dilation, so it changes the
conic gradients by at most 1e-7 / 0.09^2 ~ 1.2e-5 relative.

`forward` returns a margin mask: the pixels where a discrete decision lies within a small relative margin of its threshold
(float32 rounding may take it either way), and every pixel a Gaussian can reach whose radius, rect edge, near-plane or
frustum-clamp decision or depth order is within margin.  Comparisons exclude those pixels and zero the upstream gradient
there, as the parity tests do with the oracle's `fragile`.
"""
import numpy as np
import torch

TILE = 16
ALPHA_MIN, T_MIN, ALPHA_MAX = 1.0 / 255.0, 1e-4, 0.99

# relative margins of the discrete decisions (float32 vs float64 of the same quantity)
M_POWER, M_ALPHA, M_T, M_RADIUS, M_RECT, M_NEAR, M_CLAMP, M_DEPTH = 1e-5, 5e-4, 1e-3, 2e-5, 1e-4, 1e-4, 1e-5, 1e-6

_SH0 = 0.28209479177387814
_SH1 = 0.4886025119029199
_SH2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
_SH3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
        1.445305721320277, -0.5900435899266435)

GRAD_NAMES = ("dL_dmean2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drotations")


def _t(a):
    return torch.as_tensor(np.asarray(a, np.float64))


def sh_eval(deg, sh, d):
    """The SH polynomial of CR/forward.cu:20-71 (before +0.5 and the clamp).  sh [N, M, 3], d [N, 3] unit directions."""
    x, y, z = d[:, 0:1], d[:, 1:2], d[:, 2:3]
    res = _SH0 * sh[:, 0]
    if deg > 0:
        res = res - _SH1 * y * sh[:, 1] + _SH1 * z * sh[:, 2] - _SH1 * x * sh[:, 3]
        if deg > 1:
            xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
            res = (res + _SH2[0] * xy * sh[:, 4] + _SH2[1] * yz * sh[:, 5] + _SH2[2] * (2 * zz - xx - yy) * sh[:, 6]
                   + _SH2[3] * xz * sh[:, 7] + _SH2[4] * (xx - yy) * sh[:, 8])
            if deg > 2:
                res = (res + _SH3[0] * y * (3 * xx - yy) * sh[:, 9] + _SH3[1] * xy * z * sh[:, 10]
                       + _SH3[2] * y * (4 * zz - xx - yy) * sh[:, 11] + _SH3[3] * z * (2 * zz - 3 * xx - 3 * yy) * sh[:, 12]
                       + _SH3[4] * x * (4 * zz - xx - yy) * sh[:, 13] + _SH3[5] * z * (xx - yy) * sh[:, 14]
                       + _SH3[6] * x * (xx - 3 * yy) * sh[:, 15])
    return res


def _near_int(v, rel):
    return np.abs(v - np.round(v)) <= rel * np.maximum(np.abs(v), 1.0)


class _Scene:
    """Per-Gaussian geometry of the visible Gaussians, as a differentiable function of the leaf inputs."""

    def __init__(self, cam, g, bg, mode, grad, scale_modifier=1.0):
        W, H = cam["W"], cam["H"]
        self.W, self.H, self.mode = W, H, mode
        self.gx, self.gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
        self.bg = _t(bg)
        P = g["means3D"].shape[0]
        self.P = P
        self.leaf = {"means3D": _t(g["means3D"]), "opacities": _t(g["opacities"]).reshape(P, 1)}
        if mode == "sh":
            # the kernel's float32 modifier times the float32 scales, formed in float64: the leaf of dL_dscales
            self.leaf.update(shs=_t(g["shs"]), scales=_t(g["scales"]) * float(np.float32(scale_modifier)),
                             rotations=_t(g["rotations"]))
            self.deg = int(g["sh_degree"])
        else:
            self.leaf.update(cov3D=_t(g["cov3D"]), colors=_t(g["colors"]))
        for v in self.leaf.values():
            v.requires_grad_(grad)
        vm = _t(cam["viewmatrix"]).reshape(4, 4)
        pm = _t(cam["projmatrix"]).reshape(4, 4)
        fx, fy = W / (2.0 * cam["tanfovx"]), H / (2.0 * cam["tanfovy"])
        limx, limy = 1.3 * cam["tanfovx"], 1.3 * cam["tanfovy"]
        campos = _t(cam["campos"])

        # which Gaussians survive preprocessing: decided without gradients
        with torch.no_grad():
            geo = self._geometry(self.leaf, vm, pm, fx, fy, limx, limy)
        self.geo_all = geo
        z, txtz, tytz = geo["t"][:, 2].numpy(), geo["txtz"].numpy(), geo["tytz"].numpy()
        rad_f = 3.0 * np.sqrt(geo["l1"].numpy())
        radius = np.ceil(rad_f)
        pix = geo["pix"].numpy()
        rect = self._rect(pix, radius)
        alive = (z > 0.2) & ((rect[2] - rect[0]) * (rect[3] - rect[1]) > 0)
        self.radii = np.where(alive, radius, 0).astype(np.int32)
        self.txtz, self.tytz, self.limx, self.limy, self.z = txtz, tytz, limx, limy, z
        # Gaussians whose discrete preprocess decisions are within margin: every pixel they may reach is fragile.  A radius or
        # rect edge near an integer counts only where the other rounding would change the clamped tile rect.
        near_n = np.round(rad_f)
        alt = np.where(_near_int(rad_f, M_RADIUS), 2 * near_n + 1 - radius, radius)
        flag = (np.abs(z - 0.2) <= M_NEAR * 0.2)
        for other in (self._rect(pix, alt), self._rect(pix, radius, M_RECT), self._rect(pix, radius, -M_RECT)):
            flag |= np.any([a != b for a, b in zip(rect, other)], axis=0)
        flag |= (np.abs(np.abs(txtz) - limx) <= M_CLAMP * limx) | (np.abs(np.abs(tytz) - limy) <= M_CLAMP * limy)
        vis = np.nonzero(alive)[0]
        order = vis[np.argsort(z[vis], kind="stable")]  # depth order (CR/rasterizer_impl.cu:302-310)
        zs = z[order]
        tie = np.zeros(len(order), bool)
        if len(order) > 1:  # neighbours in depth order closer than float32 can tell apart, whose rects overlap
            x0, y0, x1, y1 = (r[order] for r in rect)
            close = ((np.diff(zs) <= M_DEPTH * zs[1:]) & (np.maximum(x0[1:], x0[:-1]) < np.minimum(x1[1:], x1[:-1]))
                     & (np.maximum(y0[1:], y0[:-1]) < np.minimum(y1[1:], y1[:-1])))
            tie[1:] |= close
            tie[:-1] |= close
        flag[order[tie]] = True
        self.order = order
        self.flag_rect = self._rect(pix, radius + 1, slack=M_RECT)
        self.flagged = np.nonzero(flag & (z > 0.2 * (1 - M_NEAR)))[0]
        self.vm, self.pm, self.fx, self.fy, self.lims, self.campos = vm, pm, fx, fy, (limx, limy), campos
        self.rect = rect

    def _rect(self, pix, radius, slack=0.0):
        """getRect (CR/auxiliary.h:46-56) in float64; `slack` widens it for the fragile marking."""
        x0 = np.clip(np.floor((pix[:, 0] - radius) / TILE - slack), 0, self.gx)
        y0 = np.clip(np.floor((pix[:, 1] - radius) / TILE - slack), 0, self.gy)
        x1 = np.clip(np.floor((pix[:, 0] + radius + TILE - 1) / TILE + slack), 0, self.gx)
        y1 = np.clip(np.floor((pix[:, 1] + radius + TILE - 1) / TILE + slack), 0, self.gy)
        return x0.astype(np.int64), y0.astype(np.int64), x1.astype(np.int64), y1.astype(np.int64)

    def _geometry(self, L, vm, pm, fx, fy, limx, limy):
        p = L["means3D"]
        t = p @ vm[:3, :3] + vm[3, :3]  # row-vector convention (CR/auxiliary.h:58-77)
        ph = p @ pm[:3, :] + pm[3, :]
        ndc = ph[:, :2] * (1.0 / (ph[:, 3:4] + 1e-7))
        pix = ((ndc + 1.0) * torch.tensor([float(self.W), float(self.H)], dtype=torch.float64) - 1.0) * 0.5
        if self.mode == "sh":
            q, s = L["rotations"], L["scales"]
            r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
            Rq = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                              2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                              2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)
            Sig = Rq @ (s[:, :, None] ** 2 * Rq.transpose(1, 2))
            cov6 = torch.stack([Sig[:, 0, 0], Sig[:, 0, 1], Sig[:, 0, 2], Sig[:, 1, 1], Sig[:, 1, 2], Sig[:, 2, 2]], -1)
        else:
            cov6 = L["cov3D"]
        c = cov6
        V = torch.stack([c[:, 0], c[:, 1], c[:, 2], c[:, 1], c[:, 3], c[:, 4], c[:, 2], c[:, 4], c[:, 5]], -1).reshape(-1, 3, 3)
        tx, ty, tz = t[:, 0], t[:, 1], t[:, 2]
        txtz, tytz = tx / tz, ty / tz
        with torch.no_grad():
            inx, iny = txtz.abs() <= limx, tytz.abs() <= limy
            cx, cy = (txtz.clamp(-limx, limx) * tz), (tytz.clamp(-limy, limy) * tz)
        txc = torch.where(inx, tx, cx.detach())  # clamped: a constant of the backward (x_grad_mul = 0, t.x held in dL_dtz)
        tyc = torch.where(iny, ty, cy.detach())
        zero = torch.zeros_like(tz)
        J = torch.stack([fx / tz, zero, -fx * txc / (tz * tz), zero, fy / tz, -fy * tyc / (tz * tz)], -1).reshape(-1, 2, 3)
        Rv = vm[:3, :3].T
        JW = J @ Rv
        cov2 = JW @ V @ JW.transpose(1, 2)
        a, b, cc = cov2[:, 0, 0] + 0.3, cov2[:, 0, 1], cov2[:, 1, 1] + 0.3
        det = a * cc - b * b
        conic = torch.stack([cc / det, -b / det, a / det], -1)
        mid = 0.5 * (a + cc)
        l1 = mid + torch.sqrt(torch.clamp(mid * mid - det, min=0.1))
        return dict(t=t, ndc=ndc, pix=pix, cov6=cov6, conic=conic, l1=l1, txtz=txtz, tytz=tytz)

    def per_gaussian(self):
        """Differentiable per-Gaussian quantities of the visible Gaussians, in depth order."""
        idx = torch.as_tensor(self.order)
        L = {k: v[idx] for k, v in self.leaf.items()}
        geo = self._geometry(L, self.vm, self.pm, self.fx, self.fy, *self.lims)
        if self.mode == "sh":
            d = L["means3D"] - self.campos
            d = d / torch.linalg.norm(d, dim=1, keepdim=True)
            rgb = torch.relu(sh_eval(self.deg, L["shs"], d) + 0.5)
        else:
            rgb = L["colors"]
        geo.update(rgb=rgb, opac=L["opacities"][:, 0])
        return geo


def _blend(S, geo, p0, p1, want_margin):
    """Pixels p0..p1 (row-major).  Returns color [n,3], depth [n], alpha [n] and, without gradients, the margin / stats."""
    W = S.W
    pid = np.arange(p0, p1)
    px, py = pid % W, pid // W
    x0, y0, x1, y1 = (r[S.order] for r in S.rect)
    tx, ty = px // TILE, py // TILE
    inrect = torch.as_tensor((x0[None] <= tx[:, None]) & (tx[:, None] < x1[None]) & (y0[None] <= ty[:, None])
                             & (ty[:, None] < y1[None]))
    pix, con, op = geo["pix"], geo["conic"], geo["opac"]
    dx = pix[None, :, 0] - _t(px)[:, None]
    dy = pix[None, :, 1] - _t(py)[:, None]
    power = -0.5 * (con[None, :, 0] * dx * dx + con[None, :, 2] * dy * dy) - con[None, :, 1] * dx * dy
    araw = op[None] * torch.exp(power)
    one = torch.ones((len(pid), 1), dtype=torch.float64)  # (not ones_like of a column: no Gaussian may be visible at all)
    alpha = araw - (araw - ALPHA_MAX).clamp(min=0).detach()  # min(0.99, o G) with the unclamped gradient
    with torch.no_grad():
        inc = inrect & (power <= 0) & (alpha >= ALPHA_MIN)
        a_inc = torch.where(inc, alpha, torch.zeros_like(alpha))
        Tb = torch.cumprod(torch.cat([one, 1 - a_inc[:, :-1]], 1), 1)
        test = Tb * (1 - a_inc)
        term = inc & (test < T_MIN)
        nterm = torch.cumsum(term.to(torch.int64), 1)
        keep = inc & (nterm == 0)
        out = {}
        if want_margin:
            evaluated = inrect & ((nterm - term.to(torch.int64)) == 0)
            m = (evaluated & (power.abs() <= M_POWER)).any(1)
            m |= (evaluated & (power <= 0) & ((alpha - ALPHA_MIN).abs() <= M_ALPHA * ALPHA_MIN)).any(1)
            m |= (evaluated & inc & ((test - T_MIN).abs() <= M_T * T_MIN)).any(1)
            out = dict(margin=m.numpy(), clamped=(keep & (araw > ALPHA_MAX)).any(1).numpy(), terminated=term.any(1).numpy(),
                       n_contrib=keep.sum(1).numpy())
    a_eff = torch.where(keep, alpha, torch.zeros_like(alpha))
    T = torch.cumprod(torch.cat([one, 1 - a_eff], 1), 1)
    wgt = a_eff * T[:, :-1]
    Tf = T[:, -1]
    color = wgt @ geo["rgb"] + Tf[:, None] * S.bg[None]
    depth = wgt @ geo["t"][:, 2].detach()
    return color, depth, wgt.sum(1), out


def _chunks(S, n_vis):
    N = S.W * S.H
    step = max(64, int(2e6 // max(n_vis, 1)))
    return [(p, min(N, p + step)) for p in range(0, N, step)]


def forward(cam, g, bg, mode, scale_modifier=1.0):
    """Images (float64 numpy, [3,H,W] / [1,H,W] / [1,H,W]), radii, the margin mask [H,W] and coverage statistics."""
    S = _Scene(cam, g, bg, mode, grad=False, scale_modifier=scale_modifier)
    W, H = S.W, S.H
    with torch.no_grad():
        geo = S.per_gaussian()
        parts = [_blend(S, geo, p0, p1, True) for p0, p1 in _chunks(S, len(S.order))]
    color = torch.cat([p[0] for p in parts]).numpy().T.reshape(3, H, W)
    depth = torch.cat([p[1] for p in parts]).numpy().reshape(1, H, W)
    alpha = torch.cat([p[2] for p in parts]).numpy().reshape(1, H, W)
    st = {k: np.concatenate([p[3][k] for p in parts]).reshape(H, W) for k in ("margin", "clamped", "terminated", "n_contrib")}
    margin = st["margin"].copy()
    fx0, fy0, fx1, fy1 = S.flag_rect
    pix, con, op = S.geo_all["pix"].numpy(), S.geo_all["conic"].numpy(), g["opacities"].reshape(-1)
    for i in S.flagged:  # the pixels of its (widened) rect where the Gaussian is not below the alpha cut-off
        ys, xs = np.mgrid[fy0[i] * TILE:min(H, fy1[i] * TILE), fx0[i] * TILE:min(W, fx1[i] * TILE)]
        dx, dy = pix[i, 0] - xs, pix[i, 1] - ys
        power = -0.5 * (con[i, 0] * dx * dx + con[i, 2] * dy * dy) - con[i, 1] * dx * dy
        margin[ys, xs] |= op[i] * np.exp(power) >= ALPHA_MIN * (1 - M_ALPHA)
    return dict(color=color, depth=depth, alpha=alpha, radii=S.radii, margin=margin, clamped=st["clamped"],
                terminated=st["terminated"], n_contrib=st["n_contrib"], txtz=S.txtz, tytz=S.tytz, limx=S.limx, limy=S.limy,
                z=S.z, flagged=S.flagged)


def backward(cam, g, bg, mode, dL_dcolor, dL_ddepth, dL_dalpha, scale_modifier=1.0):
    """Gradients of sum(dL_dcolor * color + dL_ddepth * depth + dL_dalpha * alpha), named and shaped as the oracle's
    (dL_dscales with respect to scale_modifier * scales, the reference kernel's convention)."""
    S = _Scene(cam, g, bg, mode, grad=True, scale_modifier=scale_modifier)
    W, H, P = S.W, S.H, S.P
    geo = S.per_gaussian()
    for k in ("ndc", "rgb", "cov6"):
        if geo[k].requires_grad and not geo[k].is_leaf:
            geo[k].retain_grad()
    dc = _t(dL_dcolor).reshape(3, H * W).T
    dd, da = _t(dL_ddepth).reshape(H * W), _t(dL_dalpha).reshape(H * W)
    chunks = _chunks(S, len(S.order))
    for j, (p0, p1) in enumerate(chunks):
        color, depth, alpha, _ = _blend(S, geo, p0, p1, False)
        loss = (color * dc[p0:p1]).sum() + (depth * dd[p0:p1]).sum() + (alpha * da[p0:p1]).sum()
        if loss.requires_grad:
            loss.backward(retain_graph=j + 1 < len(chunks))

    def full(x, shape):
        out = np.zeros(shape)
        if x is not None and len(S.order):
            out[S.order] = x.detach().numpy().reshape((len(S.order),) + shape[1:])
        return out

    def leafgrad(k, shape):
        v = S.leaf.get(k)
        return np.zeros(shape) if v is None or v.grad is None else v.grad.numpy().reshape(shape)

    out = dict(dL_dmean2D=np.zeros((P, 3)))
    out["dL_dmean2D"][:, :2] = full(geo["ndc"].grad, (P, 2))
    out["dL_dcolors"] = full(geo["rgb"].grad, (P, 3))
    out["dL_dopacity"] = leafgrad("opacities", (P, 1))
    out["dL_dmeans3D"] = leafgrad("means3D", (P, 3))
    if mode == "sh":
        out["dL_dcov3D"] = full(geo["cov6"].grad, (P, 6))
        M = g["shs"].shape[1]
        out["dL_dsh"] = leafgrad("shs", (P, M, 3))
        out["dL_dscales"] = leafgrad("scales", (P, 3))
        out["dL_drotations"] = leafgrad("rotations", (P, 4))
    else:
        out["dL_dcov3D"] = leafgrad("cov3D", (P, 6))
    return out


def upstream(H, W, seed, keep):
    """Seeded upstream gradients (color, depth, alpha), zero outside `keep` [H, W]."""
    rng = np.random.default_rng(seed + 50)
    k = keep.astype(np.float32)
    return ((rng.normal(0, 1, (3, H, W)) * k).astype(np.float32), (rng.normal(0, 1, (1, H, W)) * k).astype(np.float32),
            (rng.normal(0, 1, (1, H, W)) * k).astype(np.float32))

