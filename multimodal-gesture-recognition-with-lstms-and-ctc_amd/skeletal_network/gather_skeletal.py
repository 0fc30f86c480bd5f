"""Drop-in for the reference's skeletal_network/gather_skeletal.py (implementation: activity.py)."""
from .activity import load_data  # noqa: F401
