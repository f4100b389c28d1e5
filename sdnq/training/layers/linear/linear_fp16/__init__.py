"""sdnq.training.layers.linear.linear_fp16 of the import-name drop-in (see sdnq/training/__init__.py)."""
