"""flexam_amd -- MI355X-native implementation of FlexAM's denoising hot path.

Exports the reference's names (FlexAM/models/__init__.py, FlexAM/pipeline/__init__.py) so
`pipelines.py` / ComfyUI nodes can import them unchanged:
    Wan2_2Transformer3DModel_FlexAM, WanTransformer3DModel_FlexAM, AutoencoderKLWan3_8,
    Wan2_2FunControlPipeline_FlexAM, attention
and, for the step in front of the sampler, `visualize_tracking_DELTA` (pipelines.py:1852: tracks -> conditioning videos), and the
qfloat8 helpers of FlexAM/utils/fp8_optimization.py (`convert_model_weight_to_float8`, `convert_weight_dtype_wrapper`, ...), and
demo.py's edit masks (`generate_mask_fg_tracking_for_validation`, `generate_mask_bg_tracking_for_validation`), and the edit tracks
of pipelines.py (`CameraMotionGenerator`, `ObjectMotionGenerator`, `convert_moge_to_delta_format`; `moge_tracks` fuses demo.py:222-266),
and the frames that cross the boundary (`get_maskvideo_to_video_latent`, `get_video_to_video_latent`'s tensor branch, `resize_frames`,
`frames_to_bytes`: flexam_amd/frames.py), and FlexAM/utils/lora_utils.py's `merge_lora` / `unmerge_lora` (flexam_amd/lora_utils.py).
Arithmetic runs in libflexam_hip.so (hand-written gfx950 HIP kernels, C ABI in
include/flexam_hip.h); this package is the host-side mirror of the reference interface.
"""
__all__ = ["Wan2_2Transformer3DModel_FlexAM", "WanTransformer3DModel_FlexAM", "AutoencoderKLWan3_8",
           "Wan2_2FunControlPipeline_FlexAM", "FlowMatchEulerDiscreteScheduler", "FlowUniPCMultistepScheduler",
           "FlowDPMSolverMultistepScheduler", "WanT5EncoderModel", "attention", "visualize_tracking_DELTA",
           "replace_parameters_by_name", "convert_model_weight_to_float8", "autocast_model_forward", "convert_weight_dtype_wrapper",
           "generate_mask_fg_tracking_for_validation", "generate_mask_bg_tracking_for_validation",
           "CameraMotionGenerator", "ObjectMotionGenerator", "convert_moge_to_delta_format", "moge_tracks",
           "resize_tables", "resize_frames", "frames_to_bytes", "get_maskvideo_to_video_latent", "get_video_to_video_latent",
           "merge_lora", "unmerge_lora"]


def __getattr__(name):
    # lazy: importing the package must not need torch.cuda or the built library
    if name in ("Wan2_2Transformer3DModel_FlexAM", "WanTransformer3DModel_FlexAM"):
        from . import wan_transformer3d_FlexAM as m
        return getattr(m, name)
    if name == "AutoencoderKLWan3_8":
        from .wan_vae3_8 import AutoencoderKLWan3_8
        return AutoencoderKLWan3_8
    if name in ("Wan2_2FunControlPipeline_FlexAM", "WanPipelineOutput"):
        from . import pipeline_wan2_2_fun_control_FlexAM as m
        return getattr(m, name)
    if name == "FlowMatchEulerDiscreteScheduler":
        from .scheduler import FlowMatchEulerDiscreteScheduler
        return FlowMatchEulerDiscreteScheduler
    if name == "FlowUniPCMultistepScheduler":
        from .fm_solvers_unipc import FlowUniPCMultistepScheduler
        return FlowUniPCMultistepScheduler
    if name == "FlowDPMSolverMultistepScheduler":
        from .fm_solvers import FlowDPMSolverMultistepScheduler
        return FlowDPMSolverMultistepScheduler
    if name == "WanT5EncoderModel":
        from .wan_text_encoder import WanT5EncoderModel
        return WanT5EncoderModel
    if name == "attention":
        from .attention_utils import attention
        return attention
    if name in ("replace_parameters_by_name", "convert_model_weight_to_float8", "autocast_model_forward", "convert_weight_dtype_wrapper"):
        from . import fp8_optimization as m
        return getattr(m, name)
    if name == "visualize_tracking_DELTA":
        from .conditioning_raster import visualize_tracking_DELTA
        return visualize_tracking_DELTA
    if name in ("generate_mask_fg_tracking_for_validation", "generate_mask_bg_tracking_for_validation"):
        from . import edit_masks as m
        return getattr(m, name)
    if name in ("CameraMotionGenerator", "ObjectMotionGenerator", "convert_moge_to_delta_format", "moge_tracks"):
        from . import motion as m
        return getattr(m, name)
    if name in ("resize_tables", "resize_frames", "frames_to_bytes", "get_maskvideo_to_video_latent", "get_video_to_video_latent"):
        from . import frames as m
        return getattr(m, name)
    if name in ("merge_lora", "unmerge_lora"):
        from . import lora_utils as m
        return getattr(m, name)
    raise AttributeError(name)
