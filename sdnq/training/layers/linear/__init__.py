"""sdnq.training.layers.linear of the import-name drop-in (see sdnq/training/__init__.py)."""
