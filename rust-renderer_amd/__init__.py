"""rust-renderer_amd — MI355X-native path-tracing + ReSTIR core (drop-in for the reference's
reference_pt_pass + ReSTIR reservoir passes). Host mirror of the reference surface in api.py,
HIP kernels + C ABI in csrc/ (built to libutopian_hip.so by build.py)."""
from . import camera, distributed, gltf, launch, scenes, types  # noqa: F401
from .api import (  # noqa: F401
    FrameLoop,
    MultiGpuRenderer,
    Renderer,
    UtopianError,
    area_light_default_params,
    default_denoise_params,
    default_view,
    fog_default_params,
    glass_default_params,
    glossy_default_params,
    hip_versions,
    identity3x4,
    load_library,
    make_light,
    make_material,
    post_default_params,
    post_level_size,
    rtao_default_params,
    rtgi_default_params,
    shadow_cascades,
    taa_default_params,
    taa_jitter,
    transform3x4,
)
from .build import build_library  # noqa: F401
from .types import *  # noqa: F401,F403
