"""Drop-in for the reference's skeletal_network/velocity.py (implementation: activity.py)."""
from .activity import calculate_hand_velocities  # noqa: F401
