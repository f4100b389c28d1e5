"""sdnq.kernels of the import-name drop-in: the attention entry points of the reference's kernels package (see sdnq/__init__.py)."""
