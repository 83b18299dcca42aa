"""CPU restatement of the hybrid frame's deferred pass with its features together (k_hybrid_deferred<kIbl, kShadow, kRestir>, all eight
instantiations): deferred.frag in numpy float32 with the ambient term from the IBL maps or the constant, the shadow factor from the
cascaded shadow maps or from rt_shadows, and the light loop over the view's lights or over the sun plus the spatial reservoir's light.
Nothing is computed here that is not computed in the restatements of the features one at a time; this module only puts their pieces in
the kernel's order:
  hybrid_restir_reference.surface_terms, sum_lights, reservoir_term   the light loop, split where hybrid_shading.h splits it
  ibl_reference.image_based_lighting                                    pbr_lighting.glsl:81-108
  shadow_map_reference.calculate_shadow                                 shadow_mapping.glsl
  hybrid_frame_reference.unorm_lut, gamma_table                         the UNORM8 reads
tests/test_hybrid_compose_cpu.py holds it to each of those restatements, on that restatement's own domain, bit for bit. Each input image
is an argument, so a test can feed it the device's own. Not a conftest: test modules import it."""
import numpy as np

import hybrid_frame_reference as fr
import hybrid_restir_reference as rl
import ibl_reference as ir
import shadow_map_reference as sr

F = np.float32


def shadow_factor(g, view, shadow):
    """calculateShadow at every pixel's G-buffer position for shadow = (params, maps): (factor (n,), cascade (n,))"""
    params, maps = shadow
    return sr.calculate_shadow(g["position"][..., :3].reshape(-1, 3).astype(np.float32), view, params, maps)


def deferred(g, shadows, reflections, ssao_img, view, meshes, lights, maps=None, shadow=None, res=None, vis=None):
    """deferred.frag: (H, W, 4) float32. maps: the IBL maps of ibl_reference.read_maps (ibl_enabled = 1); shadow: (params, maps) as
    forward_reference.forward takes it (shadows_enabled = 1); res, vis: the spatial reservoirs and the light-visibility image
    (UH_HYBRID_RESTIR_LIGHTS). In the kernel's order: Lo, the ambient term, their sum, the metal mix, one shadow factor, SSAO."""
    assert (res is None) == (vis is None)
    s = rl.surface_terms(g, view, meshes)
    H, W = s["shape"]
    with np.errstate(all="ignore"):
        if res is None:
            Lo = rl.sum_lights(s, fr.light_records(view, list(lights)[: view.num_lights]))
        else:  # the sun alone, then the reservoir's light where its ray arrived
            Lo = rl.sum_lights(s, fr.light_records(view, [])[:1])
            term, lit = rl.reservoir_term(s, view, lights, res, vis)
            Lo = np.where(lit[:, None], Lo + term, Lo)
        if maps is None:
            ambient = (F(0.03) * s["diffuse"]) * s["occlusion"][:, None]
        else:
            ambient = ir.image_based_lighting(maps, s["P"], s["base"], s["N"], s["metallic"], s["roughness"], s["occlusion"], view.eye_pos[:])
        color = ambient + Lo
        rt = view.raytracing_supported == 1
        if rt:
            refl = fr.unorm_lut(reflections.reshape(-1, 4)[:, :3])
            color = np.where((s["type"] == 1.0)[:, None], color * (F(1.0) - F(1.0)) + refl * F(1.0), color)
        if shadow is not None:  # one factor or the other, never both
            color = color * shadow_factor(g, view, shadow)[0][:, None]
        elif rt:
            color = color * np.maximum(fr.unorm_lut(shadows.reshape(-1)), F(0.3))[:, None]
        if view.ssao_enabled == 1:
            color = color * (ssao_img[::-1].reshape(-1).astype(np.float32) / F(65535.0))[:, None]
    out = np.ones((s["n"], 4), np.float32)
    out[:, :3] = color
    return out.reshape(H, W, 4)
