"""The reference's skeletal_network/extract_activity_feats.py, continued through gather_skeletal.py and skeletal_feature_extraction.py:
``python -m mgr_amd.skeletal_network.extract_activity_feats --in <joint files> --out <dir>`` writes Training_set_skeletal.csv and
Validation_set_skeletal.csv (implementation: activity.py)."""
from .activity import extract_activity, main, skeletal_tables  # noqa: F401

if __name__ == '__main__':
    main()
