"""The reference's import path `from src.text_encoder import encode_prompt`, served by the HIP text encoders."""
from unigen_amd.text import CLIPTextModel, T5EncoderModel, encode_prompt  # noqa: F401
