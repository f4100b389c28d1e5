"""sdnq.training of the import-name drop-in: the int8 dynamic training Linear of ``sdnq_amd.training`` at the reference's module paths
(``sdnq.training.layers.linear.linear_int8.linear_int8_dynamic`` / ``..._dynamic_ckpt``); no arithmetic lives here.  The rest of the
reference's training package (SDNQTensor, the fp8 / uint8 / fp16 / static matmuls) is not built; its optimizer package is ``sdnq.optim``
(``sdnq_amd.optim``: AdamW on one fused launch per parameter)."""
