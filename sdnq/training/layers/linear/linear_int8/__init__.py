"""sdnq.training.layers.linear.linear_int8 of the import-name drop-in (see sdnq/training/__init__.py)."""
