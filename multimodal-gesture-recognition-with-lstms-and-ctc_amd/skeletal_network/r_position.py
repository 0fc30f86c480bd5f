"""Drop-in for the reference's skeletal_network/r_position.py (implementation: activity.py)."""
from .activity import calc_distance_from_rp, estimate_rest_position  # noqa: F401
