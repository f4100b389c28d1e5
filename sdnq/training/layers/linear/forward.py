"""sdnq.training.layers.linear.forward of the import-name drop-in: views of ``sdnq_amd.training``.

The reference's module holds ``QuantizedLinearBackward`` / ``quantized_linear_with_backward(input, weight, bias)``: F.linear on
``weight.dequantize()`` with grad_input, grad_weight and grad_bias.  What is built here differs in two ways:

  * ``quantized_linear_input_grad(layer, input)`` takes the quantized MODULE, not an ``SDNQTensor``: the forward is the module's own
    accelerated forward (its output bits are the inference call's), and the backward reads the module's stored codes;
  * there is no grad_weight: the quantized weight, its scale, zero point and SVD factors are frozen.  grad_input is
    ``grad_output @ weight.dequantize()``; grad_bias is ``grad_output.sum(0)`` when the bias requires grad.

``sdnq_amd.enable_input_grad(model)`` routes the calls of a whole model through it.
"""
from sdnq_amd.training import QuantizedLinearInputGrad, quantized_linear_input_grad  # noqa: F401
