"""The reference's import path `from src.condition import Condition, condition_dict` (and this package's `deblurring_image` and `depth_image`), served by the HIP image front end."""
from unigen_amd.condition import Condition, condition_dict, deblurring_image, depth_image  # noqa: F401
