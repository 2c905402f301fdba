"""Generate tests/golden/pbr_*.npz (CPU) from the reference's OWN pbr/light.py and pbr/shade.py, so that the shading
composition, the mip chain, the roughness schedule and get_mip are pinned by the reference's code, not by ours.

    python tests/golden/make_golden_pbr.py /path/to/reference

The reference imports native modules that do not exist here; they are stood in for in sys.modules before its pbr package is
imported:
  * nvdiffrast.torch.texture and pbr.renderutils.{diffuse,specular}_cubemap -> the float64 restatement (tests/pbr_reference.py);
  * cv2 and torchvision (imported at module top, used only to write images) -> empty modules.
light.py hard-codes device="cuda" and a float32 gradient buffer in cubemap_mip.backward (:40-44, :76-80, :127-128): its module's
`torch` name is pointed at a shim whose rand / zeros / linspace drop the device and build float64 CPU tensors; everything else
is torch itself.  The LUT (pbr/brdf_256_256.bin) is copied as data to tests/golden/pbr_brdf_256_256.bin.  The inputs are not
stored: tests/pbr_reference.py fixture_inputs() rebuilds them bit for bit; the outputs are stored as float32."""
import os
import shutil
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import pbr_reference as R  # noqa: E402


class _TorchShim(types.ModuleType):
    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def _cpu64(kw):
        kw.pop("device", None)
        kw["dtype"] = torch.float64
        return kw

    def rand(self, *a, **kw):
        return torch.rand(*a, **self._cpu64(kw))

    def zeros(self, *a, **kw):
        return torch.zeros(*a, **self._cpu64(kw))

    def linspace(self, *a, **kw):
        return torch.linspace(*a, **self._cpu64(kw))


def import_reference(ref_root):
    dr = types.ModuleType("nvdiffrast.torch")
    dr.texture = R.texture
    nv = types.ModuleType("nvdiffrast")
    nv.torch = dr
    ru = types.ModuleType("pbr.renderutils")
    ru.diffuse_cubemap = R.diffuse_cubemap
    ru.specular_cubemap = R.specular_cubemap
    sys.modules.update({"nvdiffrast": nv, "nvdiffrast.torch": dr, "pbr.renderutils": ru,
                        "cv2": types.ModuleType("cv2"), "torchvision": types.ModuleType("torchvision")})
    sys.path.insert(0, ref_root)
    import pbr.light as light
    import pbr.shade as shade
    light.torch = _TorchShim("torch")
    return light, shade


def main(ref_root):
    light_mod, shade = import_reference(ref_root)
    src_lut = os.path.join(ref_root, "pbr", "brdf_256_256.bin")
    shutil.copyfile(src_lut, os.path.join(HERE, "pbr_brdf_256_256.bin"))
    lut = torch.from_numpy(np.fromfile(src_lut, dtype=np.float32).reshape(1, 256, 256, 2).astype(np.float64))

    torch.manual_seed(0)
    inp = R.fixture_inputs()  # rebuilt by the tests: only the outputs below are stored
    out = {}
    # base 32: build_mips + pbr_shading, four flag combinations
    light = light_mod.CubemapLight(base_res=32)
    base0 = inp["base32"]
    px = {k[3:]: v for k, v in inp.items() if k.startswith("px_")}
    H, W = px["normals"].shape[:2]
    wts = {k[2:]: v for k, v in inp.items() if k.startswith("w_")}
    for case, (tone, gamma, use_met) in {"plain": (False, False, False), "tone": (True, False, False),
                                         "gamma": (False, True, False), "metallic": (False, False, True)}.items():
        with torch.no_grad():
            light.base.copy_(torch.from_numpy(base0))
        light.base.grad = None
        light.build_mips()
        t = {k: torch.from_numpy(v).requires_grad_(k not in ("normals", "view_dirs", "mask")) for k, v in px.items()}
        res = shade.pbr_shading(light=light, normals=t["normals"], view_dirs=t["view_dirs"], albedo=t["albedo"],
                                roughness=t["roughness"], mask=t["mask"], tone=tone, gamma=gamma, occlusion=t["occlusion"],
                                metallic=t["metallic"] if use_met else None, brdf_lut=lut)
        loss = sum((res[k].reshape(H, W, 3) * torch.from_numpy(w)).sum() for k, w in wts.items())
        loss.backward()
        for k in wts:
            out[f"{case}_{k}"] = res[k].detach().reshape(H, W, 3).numpy()
        for k in ("albedo", "roughness", "occlusion") + (("metallic",) if use_met else ()):
            out[f"{case}_d_{k}"] = t[k].grad.numpy()
        if case in ("plain", "metallic"):  # the light's gradient: once without and once with metallic
            out[f"{case}_d_base"] = light.base.grad.numpy()
    # base 16: the reference's build_mips divides by len(specular) - 2 = 0 there (ZeroDivisionError); the prefilter pieces
    # and export_envmap are pinned one by one instead
    light16 = light_mod.CubemapLight(base_res=16)
    base16 = inp["base16"]
    with torch.no_grad():
        light16.base.copy_(torch.from_numpy(base16))
    try:
        light16.build_mips()
        raise AssertionError("the reference's build_mips ran at base 16")
    except ZeroDivisionError:
        pass
    b = torch.from_numpy(base16).requires_grad_(True)
    w16 = {k[4:]: v for k, v in inp.items() if k.startswith("w16_")}
    mip = light_mod.cubemap_mip.apply(b)
    dif = R.diffuse_cubemap(b)
    spe = R.specular_cubemap(b, 0.5)
    light16.base = torch.nn.Parameter(b.detach().clone())
    env = light16.export_envmap(return_img=True, res=[16, 32])
    for k, t in (("mip", mip), ("diffuse", dif), ("specular", spe)):
        out[f"b16_{k}"] = t.detach().numpy()
        g, = torch.autograd.grad((t * torch.from_numpy(w16[k])).sum(), b)
        out[f"b16_d_{k}"] = g.numpy()
    out["b16_envmap"] = env.detach().numpy()
    g, = torch.autograd.grad((env * torch.from_numpy(w16["envmap"])).sum(), light16.base)
    out["b16_d_envmap"] = g.numpy()
    # float32 storage keeps the file small; the inputs are float32 values already, and 1e-7 is far inside every tolerance
    np.savez_compressed(os.path.join(HERE, "pbr_light.npz"), **{k: v.astype(np.float32) for k, v in out.items()})
    print("wrote", os.path.join(HERE, "pbr_light.npz"), len(out), "arrays")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("REFERENCE_ROOT", "."))
