"""sdnq.training.layers of the import-name drop-in (see sdnq/training/__init__.py)."""
