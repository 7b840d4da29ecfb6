"""The reference's import path `from src.condition import Condition, condition_dict`, served by the HIP image front end."""
from unigen_amd.condition import Condition, condition_dict  # noqa: F401
