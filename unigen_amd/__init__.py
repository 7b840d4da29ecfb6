"""unigen_amd: MI355X-native (gfx950) implementation of UniGen's condition-weaving + expert-modulation forward pass.

Layout: csrc/ (HIP kernels + C ABI -> libunigen_hip.so), lib.py (ctypes binding), ops.py (tensor front end),
flux.py (UniGenFlux / MultiCondtionUniGenFlux host engine), pipeline.py (denoise loop / UniGenFLUXPipeline surface)."""
__version__ = "0.1.0"

# the training surface, the text encoders and the Sana transformer, imported on first use (importing the package itself needs neither torch nor the HIP library)
_LAZY = {"FlowMatchObjective": "objective", "train_step": "objective", "training_sigmas": "objective", "sample_density": "objective",
         "T5EncoderModel": "text", "CLIPTextModel": "text", "encode_prompt": "text", "CLIPTextModelWithProjection": "text",
         "encode_prompt_sd3": "text", "encode_condition_prompt_sd3": "text",
         "SanaTransformerBlock": "sana", "SanaTransformer2DModel": "sana",
         "Gemma2Model": "gemma", "encode_prompt_sana": "gemma", "AutoencoderDC": "dcae",
         "SanaPipeline": "sana_pipeline", "SanaPipelineOutput": "sana_pipeline", "DPMSolverMultistepScheduler": "sana_pipeline",
         "sana_denoise_loop": "sana_pipeline"}
__all__ = sorted(_LAZY)


def __getattr__(name):
    if name in _LAZY:
        import importlib
        return getattr(importlib.import_module(f".{_LAZY[name]}", __name__), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
