"""Drop-in for the reference's skeletal_network/load_skeleton.py (implementation: activity.py)."""
from .activity import import_data, modify_array  # noqa: F401
