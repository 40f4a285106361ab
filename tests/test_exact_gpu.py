"""Bit-exact tests of every gather-GEMM, weight-gradient and image-side kernel (through the C ABI) on integer data.

Small integers with every partial sum below 2^24: every product and every partial sum is then exact in fp32 whatever the
summation order, split-K factor, tile shape or wave schedule, bf16 storage of the operands is exact and the bf16x3 split is
(hi = x, lo = 0).  There is one right answer: f32 / bf16x3 outputs equal the reference bit for bit, bf16 outputs equal its
round-to-nearest-even, BatchNorm statistics (taken from the fp32 accumulators) equal the exact integer sums, weight gradients
and split-K slabs equal the reference.  The reference is F.conv2d / F.conv_transpose2d / a matrix product in fp32 on the CPU:
each case first asserts conv(|x|, |w|).max() < 2^24, which bounds every partial sum of the REFERENCE in any order too, so its
fp32 result is the exact integer result (the same argument that makes the kernels' answer unique).

Data: weights have a fixed number t of +-1 entries per output row (per output parity for the transposed conv), activations are
sparse ternary values times magnitudes 1..3; t follows from a target output variance (64, less where the per-channel sum of
squares has to stay below 2^24).  Where even variance 20 would overflow that sum (more than ~500k output rows per channel) the
activations are dense ODD values (+-1, rarely up to +-41) against t = 3 taps: interior outputs are odd, never zero, with a mean
square of ~6.  Each case asserts on the CPU, before any launch: the 2^24 bounds, >= 32 distinct output values, <= 10 % zeros.

Every case names the kernel it is meant for and asserts jck_last_launch() after the call; test_every_kernel_has_an_exact_case
compares the table with jck_launch_name(i).  Outputs, statistics and workspaces are views into larger allocations whose guard
regions (a NaN bit pattern, compared as integers) must come back untouched.

Cost: the CPU references dominate (about 3.5 minutes for all cases on 16 threads); the three precisions of a case share one.
"""
import ctypes
import functools
import os
import re
import zlib

import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu
PREC_NAME = {0: "bf16", 1: "f32", 2: "bf16x3"}
DT = {0: torch.bfloat16, 1: torch.float32, 2: torch.float32}
LIM = float(2 ** 24)
GUARD = 4096
PAT = {2: 0x7FC1, 4: 0x7FC12345}          # NaN bit patterns (bf16 / fp32): an unwritten output can never equal a reference
IDT = {2: torch.int16, 4: torch.int32}


@pytest.fixture(scope="module")
def G():
    import gpu_util
    return gpu_util


# ---------------------------------------------------------------------------------------------------------------------
# the table.  (op, dims, options, (kernel for bf16, f32, bf16x3)); B = 256 at image size 64, B = 128 at image size 128.
#   down  (N, Hb, Cb, Cs)   jck_conv_down / jck_conv_down_grouped (options: stats, group = images per BatchNorm group)
#   up    (N, Hs, Cs, Cb)   jck_conv_up / jck_conv_up_grouped     (options: stats, group, tanh)
#   wgrad (N, Hb, Cb, Cs)   jck_conv_wgrad, accumulate 0 and 1    (option: tune = knob forced to 0 for the case)
#   g1    (B, Ci, CiPad, Co) jck_g1_fwd with statistics;  g1w: jck_g1_wgrad
#   lin   (B, K, Kpad, N, NStore, ksplit, bias) jck_linear_fwd;  linw (B, N, K, Kpad, ldgy, permC, permHW) jck_linear_wgrad + unperm
# ---------------------------------------------------------------------------------------------------------------------
CASES = [
    # (a) the edge shapes of tests/test_ops_gpu.py: ragged image counts, Cb = 3, Cs off its padded rows, M % 64 != 0
    ("down", (3, 64, 3, 64), {"stats": True}, ('img_down', 'igemm<f32,64,128,img>', 'igemm<bf16x3,64,128,img>')),
    ("down", (5, 32, 64, 128), {"stats": True}, ('igemm_dma_persist<128,64,4>', 'igemm<f32,128,64>', 'igemm<bf16x3,128,64>')),
    ("down", (3, 32, 3, 64), {"stats": True}, ('img_down', 'igemm<f32,64,128,img>', 'igemm<bf16x3,64,128,img>')),
    ("down", (7, 8, 64, 128), {"stats": True}, ('igemm_dma_persist<128,64,4>', 'igemm<f32,128,64>', 'igemm<bf16x3,128,64>')),
    ("down", (9, 16, 64, 64), {"stats": True}, ('igemm_dma_persist<64,128,4>', 'igemm<f32,64,128>', 'igemm<bf16x3,64,128>')),
    ("down", (21, 8, 64, 64), {"stats": True}, ('igemm_dma_persist<64,128,4>', 'igemm<f32,64,128>', 'igemm<bf16x3,64,128>')),
    ("down", (5, 8, 64, 192), {}, ('igemm_dma_persist<128,64,4>', 'igemm<f32,128,64>', 'igemm<bf16x3,128,64>')),
    ("down", (1, 4, 64, 128), {"stats": True}, ('igemm_dma_persist<128,64,4>', 'igemm<f32,128,64>', 'igemm<bf16x3,128,64>')),
    ("up", (5, 4, 128, 64), {"stats": True}, ('igemm_dma_persist<64,128,4>', 'igemm<f32,64,128>', 'igemm<bf16x3,64,128>')),
    ("up", (3, 16, 128, 64), {"stats": True}, ('igemm_dma_persist<64,128,4>', 'igemm<f32,64,128>', 'igemm<bf16x3,64,128>')),
    ("up", (7, 8, 256, 128), {"stats": True}, ('igemm_dma_persist<128,64,4>', 'igemm<f32,128,64>', 'igemm<bf16x3,128,64>')),
    ("up", (9, 4, 64, 32), {"stats": True}, ('igemm_dma_persist<64,128,4>', 'igemm<f32,64,128>', 'igemm<bf16x3,64,128>')),
    ("up", (21, 4, 64, 16), {"stats": True}, ('igemm<bf16,16,256>', 'igemm<f32,16,256>', 'igemm<bf16x3,16,256>')),
    ("up", (3, 16, 64, 3), {"tanh": True}, ('img_up', 'igemm<f32,16,256>', 'igemm<bf16x3,16,256>')),
    ("up", (1, 64, 64, 3), {"tanh": True}, ('img_up', 'igemm<f32,16,256>', 'igemm<bf16x3,16,256>')),
    ("up", (5, 4, 128, 3), {"tanh": True}, ('igemm<bf16,16,256>', 'igemm<f32,16,256>', 'igemm<bf16x3,16,256>')),
    ("wgrad", (3, 64, 3, 64), {}, ('wgrad<bf16,64,64,img>', 'wgrad<f32,64,64,img>', 'wgrad<bf16x3,64,64,img>')),
    ("wgrad", (7, 8, 64, 128), {}, ('wgrad_dma<3,ws>', 'wgrad<f32,128,128>', 'wgrad<bf16x3,128,128>')),
    ("wgrad", (3, 64, 64, 128), {}, ('wgrad_dma<3,ws>', 'wgrad<f32,128,128>', 'wgrad<bf16x3,128,128>')),
    ("wgrad", (9, 16, 32, 64), {}, ('wgrad<bf16,128,64>', 'wgrad<f32,128,64>', 'wgrad<bf16x3,128,64>')),
    ("wgrad", (5, 8, 32, 192), {}, ('wgrad<bf16,128,128>', 'wgrad<f32,128,128>', 'wgrad<bf16x3,128,128>')),
    ("wgrad", (21, 8, 64, 64), {}, ('wgrad<bf16,128,64>', 'wgrad<f32,128,64>', 'wgrad<bf16x3,128,64>')),
    ("g1", (5, 200, 256, 512), {}, ('igemm_dma_persist<128,64,4>', 'igemm<f32,128,64>', 'igemm<bf16x3,128,64>')),
    ("g1", (8, 100, 128, 512), {}, ('igemm_dma_persist<128,64,4>', 'igemm<f32,128,64>', 'igemm<bf16x3,128,64>')),
    ("g1w", (5, 200, 256, 512), {}, ('wgrad_dma<3,ws>', 'wgrad<f32,128,128>', 'wgrad<bf16x3,128,128>')),
    ("g1w", (21, 100, 128, 512), {}, ('wgrad_dma<3,ws>', 'wgrad<f32,128,128>', 'wgrad<bf16x3,128,128>')),
    # (b) engine shapes, image size 64, B = 256 (csrc/engine.hip: make_topo)
    # d_convs_forward: jck_conv_down_grouped over N = B (per-pass, and the real group of a split batched pass), 2B (fake + penalty), 3B
    ("down", (256, 64, 3, 64), {"stats": True, "group": 256}, ('img_down', 'igemm<f32,64,128,img>', 'igemm<bf16x3,64,128,img>')),
    ("down", (512, 64, 3, 64), {"stats": True, "group": 256}, ('img_down', 'igemm<f32,64,128,img>', 'igemm<bf16x3,64,128,img>')),
    ("down", (768, 64, 3, 64), {"stats": True, "group": 256}, ('img_down', 'igemm<f32,64,128,img>', 'igemm<bf16x3,64,128,img>')),
    ("down", (256, 32, 64, 128), {"stats": True, "group": 256}, ('igemm_dma_persist<128,256,8>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    ("down", (512, 32, 64, 128), {"stats": True, "group": 256}, ('igemm_dma_persist<128,256,8>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    ("down", (768, 32, 64, 128), {"stats": True, "group": 256}, ('igemm_dma_persist<128,256,8>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    ("down", (256, 16, 128, 256), {"stats": True, "group": 256}, ('igemm_dma_persist<128,128,4>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    ("down", (512, 16, 128, 256), {"stats": True, "group": 256}, ('igemm_dma_persist<128,256,8>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    ("down", (768, 16, 128, 256), {"stats": True, "group": 256}, ('igemm_dma_persist<128,128,4>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    ("down", (256, 8, 256, 512), {"stats": True, "group": 256}, ('igemm_dma_persist<128,64,4>', 'igemm<f32,128,64>', 'igemm<bf16x3,128,64>')),
    ("down", (512, 8, 256, 512), {"stats": True, "group": 256}, ('igemm_dma_persist<128,128,4>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    ("down", (768, 8, 256, 512), {"stats": True, "group": 256}, ('igemm_dma_persist<128,128,4>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    # d_convs_backward: dgrad jck_conv_up over N = G * B, G = 1 (per-pass), 2, 3 (batched); D.conv1's image gradient over N = B
    ("up", (256, 32, 64, 3), {}, ('img_up', 'igemm<f32,16,256>', 'igemm<bf16x3,16,256>')),
    ("up", (256, 16, 128, 64), {}, ('igemm_dma_persist<64,128,4>', 'igemm<f32,64,128>', 'igemm<bf16x3,64,128>')),
    ("up", (512, 16, 128, 64), {}, ('igemm_dma_persist<64,128,4>', 'igemm<f32,64,128>', 'igemm<bf16x3,64,128>')),
    ("up", (768, 16, 128, 64), {}, ('igemm_dma_persist<64,128,4>', 'igemm<f32,64,128>', 'igemm<bf16x3,64,128>')),
    ("up", (256, 8, 256, 128), {}, ('igemm_dma_persist<128,256,8>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    ("up", (512, 8, 256, 128), {}, ('igemm_dma_persist<128,256,8>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    ("up", (768, 8, 256, 128), {}, ('igemm_dma_persist<128,256,8>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    ("up", (256, 4, 512, 256), {}, ('igemm_dma_persist<128,128,4>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    ("up", (512, 4, 512, 256), {}, ('igemm_dma_persist<128,256,8>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    ("up", (768, 4, 512, 256), {}, ('igemm_dma_persist<128,128,4>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    # d_convs_backward / g_backward / the penalty's double backward: jck_conv_wgrad over N = gw * B, gw = 1, 2
    ("wgrad", (256, 64, 3, 64), {}, ('wgrad<bf16,64,64,img>', 'wgrad<f32,64,64,img>', 'wgrad<bf16x3,64,64,img>')),
    ("wgrad", (512, 64, 3, 64), {}, ('wgrad<bf16,64,64,img>', 'wgrad<f32,64,64,img>', 'wgrad<bf16x3,64,64,img>')),
    ("wgrad", (256, 32, 64, 128), {}, ('wgrad_dma<3,ws>', 'wgrad<f32,128,128>', 'wgrad<bf16x3,128,128>')),
    ("wgrad", (512, 32, 64, 128), {}, ('wgrad_dma<3,ws>', 'wgrad<f32,128,128>', 'wgrad<bf16x3,128,128>')),
    ("wgrad", (256, 16, 128, 256), {}, ('wgrad_dma<3,ws>', 'wgrad<f32,128,128>', 'wgrad<bf16x3,128,128>')),
    ("wgrad", (512, 16, 128, 256), {}, ('wgrad_dma<3,ws>', 'wgrad<f32,128,128>', 'wgrad<bf16x3,128,128>')),
    ("wgrad", (256, 8, 256, 512), {}, ('wgrad_dma<3,ws>', 'wgrad<f32,128,128>', 'wgrad<bf16x3,128,128>')),
    ("wgrad", (512, 8, 256, 512), {}, ('wgrad_dma<3,ws>', 'wgrad<f32,128,128>', 'wgrad<bf16x3,128,128>')),
    # g_backward's dgrad and the penalty's v-chain: jck_conv_down without statistics, N = B
    ("down", (256, 64, 3, 64), {}, ('img_down', 'igemm<f32,64,128,img>', 'igemm<bf16x3,64,128,img>')),
    ("down", (256, 32, 64, 128), {}, ('igemm_dma_persist<128,256,8>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    ("down", (256, 16, 128, 256), {}, ('igemm_dma_persist<128,128,4>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    ("down", (256, 8, 256, 512), {}, ('igemm_dma_persist<128,64,4>', 'igemm<f32,128,64>', 'igemm<bf16x3,128,64>')),
    # g_forward: jck_g1_fwd, jck_conv_up_grouped (one group of B), the tanh image layer; g_backward: jck_g1_wgrad
    ("g1", (256, 100, 128, 512), {}, ('igemm_dma_persist<128,64,4>', 'igemm<f32,128,64>', 'igemm<bf16x3,128,64>')),
    ("g1w", (256, 100, 128, 512), {}, ('wgrad_dma<3,ws>', 'wgrad<f32,128,128>', 'wgrad<bf16x3,128,128>')),
    ("up", (256, 4, 512, 256), {"stats": True, "group": 256}, ('igemm_dma_persist<128,128,4>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    ("up", (256, 8, 256, 128), {"stats": True, "group": 256}, ('igemm_dma_persist<128,256,8>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    ("up", (256, 16, 128, 64), {"stats": True, "group": 256}, ('igemm_dma_persist<64,128,4>', 'igemm<f32,64,128>', 'igemm<bf16x3,64,128>')),
    ("up", (256, 32, 64, 3), {"tanh": True}, ('img_up', 'igemm<f32,16,256>', 'igemm<bf16x3,16,256>')),
    # (b) engine shapes, image size 128, B = 128 (csrc/engine.hip: make_topo)
    # d_convs_forward: jck_conv_down_grouped over N = B (per-pass, and the real group of a split batched pass), 2B (fake + penalty), 3B
    ("down", (128, 128, 3, 64), {"stats": True, "group": 128}, ('img_down', 'igemm<f32,64,128,img>', 'igemm<bf16x3,64,128,img>')),
    ("down", (256, 128, 3, 64), {"stats": True, "group": 128}, ('img_down', 'igemm<f32,64,128,img>', 'igemm<bf16x3,64,128,img>')),
    ("down", (384, 128, 3, 64), {"stats": True, "group": 128}, ('img_down', 'igemm<f32,64,128,img>', 'igemm<bf16x3,64,128,img>')),
    ("down", (128, 64, 64, 128), {"stats": True, "group": 128}, ('igemm_dma_persist<128,256,8>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    ("down", (256, 64, 64, 128), {"stats": True, "group": 128}, ('igemm_dma_persist<128,256,8>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    ("down", (384, 64, 64, 128), {"stats": True, "group": 128}, ('igemm_dma_persist<128,256,8>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    ("down", (128, 32, 128, 256), {"stats": True, "group": 128}, ('igemm_dma_persist<128,256,8>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    ("down", (256, 32, 128, 256), {"stats": True, "group": 128}, ('igemm_dma_persist<128,256,8>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    ("down", (384, 32, 128, 256), {"stats": True, "group": 128}, ('igemm_dma_persist<128,256,8>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    ("down", (128, 16, 256, 512), {"stats": True, "group": 128}, ('igemm_dma_persist<128,128,4>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    ("down", (256, 16, 256, 512), {"stats": True, "group": 128}, ('igemm_dma_persist<128,256,8>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    ("down", (384, 16, 256, 512), {"stats": True, "group": 128}, ('igemm_dma_persist<128,128,4>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    ("down", (128, 8, 512, 1024), {"stats": True, "group": 128}, ('igemm_dma_persist<128,64,4>', 'igemm<f32,128,64>', 'igemm<bf16x3,128,64>')),
    ("down", (256, 8, 512, 1024), {"stats": True, "group": 128}, ('igemm_dma_persist<128,128,4>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    ("down", (384, 8, 512, 1024), {"stats": True, "group": 128}, ('igemm_dma_persist<128,128,4>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    # d_convs_backward: dgrad jck_conv_up over N = G * B, G = 1 (per-pass), 2, 3 (batched); D.conv1's image gradient over N = B
    ("up", (128, 64, 64, 3), {}, ('img_up', 'igemm<f32,16,256>', 'igemm<bf16x3,16,256>')),
    ("up", (128, 32, 128, 64), {}, ('igemm_dma_persist<64,128,4>', 'igemm<f32,64,128>', 'igemm<bf16x3,64,128>')),
    ("up", (256, 32, 128, 64), {}, ('igemm_dma_persist<64,128,4>', 'igemm<f32,64,128>', 'igemm<bf16x3,64,128>')),
    ("up", (384, 32, 128, 64), {}, ('igemm_dma_persist<64,128,4>', 'igemm<f32,64,128>', 'igemm<bf16x3,64,128>')),
    ("up", (128, 16, 256, 128), {}, ('igemm_dma_persist<128,256,8>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    ("up", (256, 16, 256, 128), {}, ('igemm_dma_persist<128,256,8>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    ("up", (384, 16, 256, 128), {}, ('igemm_dma_persist<128,256,8>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    ("up", (128, 8, 512, 256), {}, ('igemm_dma_persist<128,256,8>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    ("up", (256, 8, 512, 256), {}, ('igemm_dma_persist<128,256,8>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    ("up", (384, 8, 512, 256), {}, ('igemm_dma_persist<128,256,8>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    ("up", (128, 4, 1024, 512), {}, ('igemm_dma_persist<128,128,4>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    ("up", (256, 4, 1024, 512), {}, ('igemm_dma_persist<128,256,8>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    ("up", (384, 4, 1024, 512), {}, ('igemm_dma_persist<128,128,4>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    # d_convs_backward / g_backward / the penalty's double backward: jck_conv_wgrad over N = gw * B, gw = 1, 2
    ("wgrad", (128, 128, 3, 64), {}, ('wgrad<bf16,64,64,img>', 'wgrad<f32,64,64,img>', 'wgrad<bf16x3,64,64,img>')),
    ("wgrad", (256, 128, 3, 64), {}, ('wgrad<bf16,64,64,img>', 'wgrad<f32,64,64,img>', 'wgrad<bf16x3,64,64,img>')),
    ("wgrad", (128, 64, 64, 128), {}, ('wgrad_dma<3,ws>', 'wgrad<f32,128,128>', 'wgrad<bf16x3,128,128>')),
    ("wgrad", (256, 64, 64, 128), {}, ('wgrad_dma<3,ws>', 'wgrad<f32,128,128>', 'wgrad<bf16x3,128,128>')),
    ("wgrad", (128, 32, 128, 256), {}, ('wgrad_dma<3,ws>', 'wgrad<f32,128,128>', 'wgrad<bf16x3,128,128>')),
    ("wgrad", (256, 32, 128, 256), {}, ('wgrad_dma<3,ws>', 'wgrad<f32,128,128>', 'wgrad<bf16x3,128,128>')),
    ("wgrad", (128, 16, 256, 512), {}, ('wgrad_dma<3,ws>', 'wgrad<f32,128,128>', 'wgrad<bf16x3,128,128>')),
    ("wgrad", (256, 16, 256, 512), {}, ('wgrad_dma<3,ws>', 'wgrad<f32,128,128>', 'wgrad<bf16x3,128,128>')),
    ("wgrad", (128, 8, 512, 1024), {}, ('wgrad_dma<3,ws>', 'wgrad<f32,128,128>', 'wgrad<bf16x3,128,128>')),
    ("wgrad", (256, 8, 512, 1024), {}, ('wgrad_dma<3,ws>', 'wgrad<f32,128,128>', 'wgrad<bf16x3,128,128>')),
    # g_backward's dgrad and the penalty's v-chain: jck_conv_down without statistics, N = B
    ("down", (128, 128, 3, 64), {}, ('img_down', 'igemm<f32,64,128,img>', 'igemm<bf16x3,64,128,img>')),
    ("down", (128, 64, 64, 128), {}, ('igemm_dma_persist<128,256,8>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    ("down", (128, 32, 128, 256), {}, ('igemm_dma_persist<128,256,8>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    ("down", (128, 16, 256, 512), {}, ('igemm_dma_persist<128,128,4>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    ("down", (128, 8, 512, 1024), {}, ('igemm_dma_persist<128,64,4>', 'igemm<f32,128,64>', 'igemm<bf16x3,128,64>')),
    # g_forward: jck_g1_fwd, jck_conv_up_grouped (one group of B), the tanh image layer; g_backward: jck_g1_wgrad
    ("g1", (128, 100, 128, 1024), {}, ('igemm_dma_persist<128,64,4>', 'igemm<f32,128,64>', 'igemm<bf16x3,128,64>')),
    ("g1w", (128, 100, 128, 1024), {}, ('wgrad_dma<3,ws>', 'wgrad<f32,128,128>', 'wgrad<bf16x3,128,128>')),
    ("up", (128, 4, 1024, 512), {"stats": True, "group": 128}, ('igemm_dma_persist<128,128,4>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    ("up", (128, 8, 512, 256), {"stats": True, "group": 128}, ('igemm_dma_persist<128,256,8>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    ("up", (128, 16, 256, 128), {"stats": True, "group": 128}, ('igemm_dma_persist<128,256,8>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    ("up", (128, 32, 128, 64), {"stats": True, "group": 128}, ('igemm_dma_persist<64,128,4>', 'igemm<f32,64,128>', 'igemm<bf16x3,64,128>')),
    ("up", (128, 64, 64, 3), {"tanh": True}, ('img_up', 'igemm<f32,16,256>', 'igemm<bf16x3,16,256>')),
    # (b) CGAN engine (image size 64, B = 256): G.conv1 on [z | one-hot] (z_pad 256); cg_head_forward: Linear(8392,256) as 12 split-K slabs over B / 3B rows; d_head_backward: its input gradient (ksplit 1) and weight gradient over B / 2B rows
    ("g1", (256, 200, 256, 512), {}, ('igemm_dma_persist<128,64,4>', 'igemm<f32,128,64>', 'igemm<bf16x3,128,64>')),
    ("g1w", (256, 200, 256, 512), {}, ('wgrad_dma<3,ws>', 'wgrad<f32,128,128>', 'wgrad<bf16x3,128,128>')),
    ("lin", (256, 8392, 8448, 256, 256, 12, 0), {}, ('igemm_dma<128,64,3,ws>', 'igemm<f32,128,64>', 'igemm<bf16x3,128,64>')),
    ("lin", (768, 8392, 8448, 256, 256, 12, 0), {}, ('igemm_dma<128,64,3,ws>', 'igemm<f32,128,64>', 'igemm<bf16x3,128,64>')),
    ("lin", (256, 256, 256, 8392, 8448, 1, 0), {}, ('igemm_dma<128,64,3,ws>', 'igemm<f32,128,64>', 'igemm<bf16x3,128,64>')),
    ("lin", (768, 256, 256, 8392, 8448, 1, 0), {}, ('igemm_dma<128,64,3,ws>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    ("linw", (256, 256, 8392, 8448, 256, 512, 16), {}, ('wgrad<bf16,128,128>', 'wgrad<f32,128,128>', 'wgrad<bf16x3,128,128>')),
    ("linw", (512, 256, 8392, 8448, 256, 512, 16), {}, ('wgrad<bf16,128,128>', 'wgrad<f32,128,128>', 'wgrad<bf16x3,128,128>')),
    # (c) shapes that reach the remaining kernels, and the knob forms
    ("lin", (300, 8392, 8448, 256, 256, 12, 0), {"tune": 'igemm_dma_ksplit'}, ('igemm<bf16,128,64>', 'igemm<f32,128,64>', 'igemm<bf16x3,128,64>')),
    ("lin", (1300, 8392, 8448, 256, 256, 12, 0), {"tune": 'igemm_dma_ksplit'}, ('igemm<bf16,128,128>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    ("lin", (21, 500, 512, 250, 256, 1, 1), {}, ('igemm_dma<128,64,3,ws>', 'igemm<f32,128,64>', 'igemm<bf16x3,128,64>')),
    ("lin", (700, 500, 512, 250, 256, 1, 1), {}, ('igemm_dma<128,64,3,ws>', 'igemm<f32,128,64>', 'igemm<bf16x3,128,64>')),
    ("linw", (65, 250, 500, 512, 264, 0, 0), {}, ('wgrad<bf16,128,128>', 'wgrad<f32,128,128>', 'wgrad<bf16x3,128,128>')),
    ("linw", (40, 64, 190, 192, 64, 0, 0), {}, ('wgrad<bf16,64,64>', 'wgrad<f32,64,64>', 'wgrad<bf16x3,64,64>')),
    ("linw", (40, 100, 250, 256, 104, 0, 0), {}, ('wgrad<bf16,128,64>', 'wgrad<f32,128,64>', 'wgrad<bf16x3,128,64>')),
    ("down", (3, 16, 3, 32), {"stats": True}, ('igemm<bf16,64,128,img>', 'igemm<f32,64,128,img>', 'igemm<bf16x3,64,128,img>')),
    ("down", (5, 16, 3, 64), {"stats": True}, ('igemm<bf16,64,128,img>', 'igemm<f32,64,128,img>', 'igemm<bf16x3,64,128,img>')),
    ("down", (2050, 8, 64, 512), {"stats": True}, ('igemm_dma<128,128,2>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    ("down", (4096, 4, 64, 512), {"stats": True}, ('igemm_dma<128,128,2>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    ("up", (4, 8, 128, 3), {"tanh": True}, ('igemm<bf16,16,256>', 'igemm<f32,16,256>', 'igemm<bf16x3,16,256>')),
    ("up", (64, 16, 128, 64), {"tanh": True}, ('igemm_dma<64,128,2>', 'igemm<f32,64,128>', 'igemm<bf16x3,64,128>')),
    ("up", (64, 32, 128, 128), {"tanh": True}, ('igemm_dma<128,256,3,ws,8>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    ("up", (8, 16, 128, 128), {"tanh": True}, ('igemm_dma<128,64,3,ws>', 'igemm<f32,128,64>', 'igemm<bf16x3,128,64>')),
    ("up", (96, 16, 256, 128), {"stats": True, "group": 32}, ('igemm_dma_persist<128,128,4>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    ("up", (48, 16, 128, 64), {"stats": True, "group": 16}, ('igemm_dma_persist<64,128,4>', 'igemm<f32,64,128>', 'igemm<bf16x3,64,128>')),
    ("up", (64, 16, 256, 128), {"stats": True, "group": 64}, ('igemm_dma_persist<128,256,8>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    ("down", (96, 32, 64, 128), {"stats": True, "group": 32}, ('igemm_dma_persist<128,64,4>', 'igemm<f32,128,64>', 'igemm<bf16x3,128,64>')),
    ("down", (192, 32, 64, 256), {"stats": True, "group": 64}, ('igemm_dma_persist<128,128,4>', 'igemm<f32,128,128>', 'igemm<bf16x3,128,128>')),
    ("down", (8, 16, 128, 256), {"stats": True, "group": 4}, ('igemm_dma_persist<128,64,4>', 'igemm<f32,128,64>', 'igemm<bf16x3,128,64>')),
    ("wgrad", (256, 16, 128, 256), {"tune": 'wgrad_ws'}, ('wgrad_dma<2>', 'wgrad<f32,128,128>', 'wgrad<bf16x3,128,128>')),
    ("wgrad", (7, 8, 64, 128), {"tune": 'wgrad_ws'}, ('wgrad_dma<2>', 'wgrad<f32,128,128>', 'wgrad<bf16x3,128,128>')),
    ("g1w", (256, 100, 128, 512), {"tune": 'wgrad_ws'}, ('wgrad_dma<2>', 'wgrad<f32,128,128>', 'wgrad<bf16x3,128,128>')),
    ("linw", (256, 256, 8392, 8448, 256, 512, 16), {"tune": 'wgrad_ws'}, ('wgrad<bf16,128,128>', 'wgrad<f32,128,128>', 'wgrad<bf16x3,128,128>')),
    ("wgrad", (256, 16, 128, 256), {"tune": 'wgrad_dma'}, ('wgrad<bf16,128,128>', 'wgrad<f32,128,128>', 'wgrad<bf16x3,128,128>')),
    ("wgrad", (7, 8, 64, 128), {"tune": 'wgrad_dma'}, ('wgrad<bf16,128,128>', 'wgrad<f32,128,128>', 'wgrad<bf16x3,128,128>')),
    ("g1w", (256, 100, 128, 512), {"tune": 'wgrad_dma'}, ('wgrad<bf16,128,128>', 'wgrad<f32,128,128>', 'wgrad<bf16x3,128,128>')),
    ("linw", (256, 256, 8392, 8448, 256, 512, 16), {"tune": 'wgrad_dma'}, ('wgrad<bf16,128,128>', 'wgrad<f32,128,128>', 'wgrad<bf16x3,128,128>')),
]


def case_id(c):
    op, dims, opt, _ = c
    return op + "-" + "x".join(str(d) for d in dims) + "".join(f"-{k}{'' if v is True else v}" for k, v in sorted(opt.items()))


def items(ops):
    """(case, prec) pairs, the three precisions of a case next to each other: they share one cached CPU reference."""
    return [pytest.param(c, p, id=f"{case_id(c)}-{PREC_NAME[p]}") for c in CASES if c[0] in ops for p in (0, 1, 2) if c[3][p]]


# ---------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------
def seed_of(op, dims):
    return zlib.crc32(repr((op,) + tuple(dims)).encode()) % 100003


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def ternary(shape, density, mag, seed):
    """sparse ternary values times magnitudes 1..mag, fp32"""
    g = _gen(seed)
    v = torch.randint(1, mag + 1, shape, generator=g, dtype=torch.int8)
    v = v * (torch.randint(0, 2, shape, generator=g, dtype=torch.int8) * 2 - 1)
    if density < 1.0:
        v = v * (torch.rand(shape, generator=g) < density)
    return v.float()


def odd_dense(shape, seed, hot=2e-3, hot_max=20):
    """dense odd values: +-1, a fraction `hot` of them +-(2j+1), j = 1..hot_max"""
    g = _gen(seed)
    v = torch.ones(shape, dtype=torch.int8)
    j = torch.randint(1, hot_max + 1, shape, generator=g, dtype=torch.int8)
    v = v + 2 * j * (torch.rand(shape, generator=g) < hot)
    return (v * (torch.randint(0, 2, shape, generator=g, dtype=torch.int8) * 2 - 1)).float()


def fixed_count(rows, k, t, seed):
    """[rows][k] with exactly t entries of +-1 per row"""
    g = _gen(seed)
    t = max(1, min(int(t), k))
    idx = torch.rand(rows, k, generator=g).topk(t, dim=1).indices
    sgn = (torch.randint(0, 2, (rows, t), generator=g) * 2 - 1).float()
    return torch.zeros(rows, k).scatter_(1, idx, sgn)


def w_down(cs, cb, t, seed):
    return fixed_count(cs, cb * 16, t, seed).view(cs, cb, 4, 4)


def w_up(cs, cb, t, seed):
    """ConvTranspose2d weight [Cs][Cb][4][4]: t entries per (output channel, output parity); parity (ph, pw) reads the taps with
    kh % 2 == 1 - ph, kw % 2 == 1 - pw - the split below only has to keep the four classes apart"""
    w = fixed_count(cb * 4, cs * 4, t, seed).view(cb, 2, 2, cs, 2, 2)          # [cb][khp][kwp][cs][khh][kwh], kh = 2 khh + khp
    return w.permute(3, 0, 4, 1, 5, 2).reshape(cs, cb, 4, 4).contiguous()


def plan(k_terms, rows_per_chan, stats):
    """(regime, t): activations 'A' sparse ternary x 1..3 (density 0.25, dense when the reduction is short) or 'B' dense odd"""
    var = 64.0
    if stats:
        var = min(var, 0.6 * LIM / rows_per_chan)
        if var < 20.0:
            return "B", 1.0, 3
    dens = 0.25 if k_terms >= 256 else 1.0
    return "A", dens, max(1, round(var / (dens * 14.0 / 3.0)))


def act(shape, regime, dens, seed):
    return odd_dense(shape, seed) if regime == "B" else ternary(shape, dens, 3, seed)


def conditions(ref, bound, what, stats_dims=None, min_distinct=32):
    """the exactness conditions, on the reference alone"""
    assert float(bound) < LIM, f"{what}: conv(|x|,|w|).max() = {float(bound)} >= 2^24 (test data bug)"
    if stats_dims is not None:
        q = float((ref.double() ** 2).sum(stats_dims).max())
        assert q < LIM, f"{what}: per-channel sum y^2 = {q} >= 2^24 (test data bug)"
    nd = int(torch.unique(ref).numel())
    zf = float((ref == 0).float().mean())
    assert nd >= min_distinct, f"{what}: only {nd} distinct output values (test data bug)"
    assert zf <= 0.10, f"{what}: {100 * zf:.1f} % zeros (test data bug)"


@functools.lru_cache(maxsize=1)
def conv_data(op, dims, stats, group, special=None):
    """(x NCHW, w, ref NCHW fp32) of a down / up case, conditions asserted"""
    n, h, c_in, c_out = dims
    seed = seed_of(op, dims)
    if op == "down":
        rows = (group or n) * (h // 2) ** 2
        k = 16 * c_in
    else:
        rows = (group or n) * 4 * h * h
        k = 4 * c_in
    if special == "tanh":                 # pre-activations in the integers -4 .. 4: four taps of +-1 against values in {0, +-1}
        x, w = ternary((n, c_in, h, h), 0.6, 1, seed), w_up(c_in, c_out, 4, seed + 1)
    elif special == "impulse":            # dense +-1 weights: the response to an input impulse speaks in every channel
        x = ternary((n, c_in, h, h), 0.25, 1, seed)
        w = ternary((c_out, c_in, 4, 4) if op == "down" else (c_in, c_out, 4, 4), 1.0, 1, seed + 1)
    elif special == "round":              # dense, biased: 256 < |y| < 4096 for most outputs
        x = ternary((n, c_in, h, h), 1.0, 3, seed).abs()
        w = ternary((c_out, c_in, 4, 4) if op == "down" else (c_in, c_out, 4, 4), 1.0, 1, seed + 1)
        w = torch.where(torch.rand(w.shape, generator=_gen(seed + 2)) < 0.6, w.abs(), -w.abs())
    else:
        regime, dens, t = plan(k, rows, stats)
        x = act((n, c_in, h, h), regime, dens, seed)
        w = w_down(c_out, c_in, t, seed + 1) if op == "down" else w_up(c_in, c_out, t, seed + 1)
    if op == "down":
        ref, bound = F.conv2d(x, w, None, 2, 1), F.conv2d(x.abs(), w.abs(), None, 2, 1).max()
    else:
        ref, bound = F.conv_transpose2d(x, w, None, 2, 1), F.conv_transpose2d(x.abs(), w.abs(), None, 2, 1).max()
    what = f"{op}{dims}"
    if special == "tanh":
        assert float(bound) <= 4 and sorted(torch.unique(ref).tolist()) == list(range(-4, 5)), f"{what}: pre-activations are not -4..4"
    elif special == "impulse":
        assert float(bound) < LIM and float(ref.abs().max()) < 250, f"{what}: outputs (and outputs + 1 tap) are not exact in bf16"
    elif special == "round":
        assert float(bound) < LIM
        a = ref.abs()
        assert float(((a > 256) & (a < 4096)).float().mean()) > 0.5, f"{what}: outputs are not mostly in (256, 4096)"
    else:
        if stats and group:
            for k0 in range(0, n, group):
                conditions(ref[k0:k0 + group], bound, what, (0, 2, 3))
        else:
            conditions(ref, bound, what, (0, 2, 3) if stats else None)
    return x, w, ref


def pair_density(m, target=150.0):
    """densities (small, big) of two 1..3-magnitude ternary operands whose products are summed over m terms"""
    e2 = (14.0 / 3.0) ** 2
    db = 1.0 if m * e2 <= 4 * target else 0.25          # short reductions: both operands dense, or most sums would have no term
    return min(1.0, target / (m * db * e2)), db


# ---------------------------------------------------------------------------------------------------------------------
# buffers with guards, comparison, messages
# ---------------------------------------------------------------------------------------------------------------------
class Guarded:
    """`numel` elements of dtype inside an allocation with GUARD elements of a fixed bit pattern before and after; the payload
    starts as the same pattern (a NaN).  check(used) also wants the payload past `used` elements untouched."""

    def __init__(self, numel, dtype, init=None):
        self.n, self.esz = int(numel), torch.empty(0, dtype=dtype).element_size()
        self.buf = torch.empty(self.n + 2 * GUARD, dtype=dtype, device="cuda")
        self.ints = self.buf.view(IDT[self.esz])
        self.ints.fill_(PAT[self.esz])
        self.t = self.buf[GUARD:GUARD + self.n]
        if init is not None:
            self.t.copy_(init.reshape(-1))

    def check(self, what, used=None):
        pat = PAT[self.esz]
        for name, region in (("before", self.ints[:GUARD]), ("after", self.ints[GUARD + self.n:]),
                             ("past the used part of", self.ints[GUARD + (self.n if used is None else int(used)):GUARD + self.n])):
            bad = torch.nonzero(region != pat)
            assert bad.numel() == 0, f"{what}: {bad.shape[0]} guard elements {name} the buffer overwritten, first at {int(bad[0])}"


def tile_of(kernel, idx, op, dims):
    """tile coordinates of an output element for the kernel that ran (tile sizes from its name: rows x pixels, or columns x rows)"""
    m = re.search(r"<(?:bf16x3,|bf16,|f32,)?(\d+),(\d+)", kernel)
    if kernel.startswith("wgrad_dma"):
        a, b = 128, 128
    elif m:
        a, b = int(m.group(1)), int(m.group(2))
    else:
        return "n/a (a streaming kernel)"
    if op == "down":
        n, oy, ox, c = idx
        oh = dims[1] // 2
        return f"(pixel tile {((n * oh + oy) * oh + ox) // b}, channel tile {c // a})"
    if op == "up":
        n, oy, ox, c = idx
        hs = dims[1]
        return f"(pixel tile {((n * hs + oy // 2) * hs + ox // 2) // b}, channel tile {c // a}, parity {(oy % 2) * 2 + ox % 2})"
    if op == "wgrad":
        co, ci, kh, kw = idx
        cbp = 4 if dims[2] == 3 else dims[2]
        return f"(column tile {((kh * 4 + kw) * cbp + ci) // a}, row tile {co // b})"
    if op == "g1":                      # rows = (tap, co), pixels = the batch
        bi, kh, kw, co = idx
        return f"(pixel tile {bi // b}, channel tile {((kh * 4 + kw) * dims[3] + co) // a})"
    if op == "lin":                     # rows = output columns, pixels = the batch rows; split-K layer = slab
        sl = f", split-K layer {idx[0]}" if len(idx) == 3 else ""
        return f"(pixel tile {idx[-2] // b}, channel tile {idx[-1] // a}{sl})"
    if op == "g1w":
        ci, co, kh, kw = idx
        return f"(column tile {((kh * 4 + kw) * dims[3] + co) // a}, row tile {ci // b})"
    if op == "linw":
        return f"(column tile {idx[1] // a}, row tile {idx[0] // b})"
    return f"(tile sizes {a} x {b})"


def expect_equal(got, ref, what, axes, kernel="", op="", dims=()):
    """got == ref bit for bit (device tensors of one dtype and shape); the message decodes the first and the worst mismatch"""
    assert got.shape == ref.shape and got.dtype == ref.dtype, f"{what}: {tuple(got.shape)} {got.dtype} vs {tuple(ref.shape)} {ref.dtype}"
    if torch.equal(got, ref):
        return
    g, r = got.double().cpu(), ref.double().cpu()
    d = torch.nan_to_num(g - r, nan=float("inf"))
    bad = torch.nonzero(d != 0)
    first = tuple(bad[0].tolist())
    worst = tuple(torch.nonzero(d.abs() == d.abs().max())[0].tolist())
    msg = [f"{what} [{kernel}]: {bad.shape[0]} of {g.numel()} elements differ"]
    for tag, i in (("first", first), ("worst", worst)):
        msg.append(f"  {tag} at {axes} = {i}, tile {tile_of(kernel, i, op, dims)}: got {g[i].item():.10g} ref {r[i].item():.10g} "
                   f"diff {d[i].item():+.10g}")
    raise AssertionError("\n".join(msg))


def ran(G, want, what):
    got = G.lib.jck_last_launch().decode()
    assert got == want, f"{what}: ran on {got}, the case was written for {want} (a dispatch threshold moved?)"


def nhwc(x_nchw, dtype, cpad=None):
    n, c, h, w = x_nchw.shape
    cp = cpad or (4 if c == 3 else c)
    if cp == c:
        return x_nchw.permute(0, 2, 3, 1).to(dtype).cuda().contiguous()
    t = torch.zeros(n, h, w, cp)
    t[..., :c] = x_nchw.permute(0, 2, 3, 1)
    return t.to(dtype).cuda().contiguous()


def pack_down(G, w, prec):
    cs, cb = w.shape[0], w.shape[1]
    wp = torch.empty(G.lib.jck_pad_rows(cs) * 16 * G.lib.jck_pad_chan(cb), dtype=DT[prec], device="cuda")
    G.lib.jck_pack_down(prec, w.cuda().contiguous(), cs, cb, wp, G.cur_stream())
    return wp


def pack_up(G, w, prec):
    cs, cb = w.shape[0], w.shape[1]
    wp = torch.empty(4 * G.lib.jck_pad_rows(cb) * 4 * cs, dtype=DT[prec], device="cuda")
    G.lib.jck_pack_up(prec, w.cuda().contiguous(), cs, cb, wp, G.cur_stream())
    return wp


def stats_rows(st, slots, c, groups):
    """[groups][rows][2][C] (double, device) of the rows the call reports"""
    per = slots // groups
    assert slots % groups == 0 and per >= 1, f"{slots} statistics rows do not split over {groups} groups"
    return st.t[:slots * 2 * c].view(groups, per, 2, c).double()


def check_stats(st, slots, c, c_real, ref, groups, what):
    rows = stats_rows(st, slots, c, groups)
    assert bool(torch.isfinite(rows).all()), f"{what}: a reported statistics row was not written"
    gi = ref.shape[0] // groups
    for k in range(groups):
        r = ref[k * gi:(k + 1) * gi].double()
        for j, (name, exp) in enumerate((("sum y", r.sum((0, 2, 3))), ("sum y^2", (r * r).sum((0, 2, 3))))):
            got = rows[k, :, j].sum(0)[:c_real].cpu()
            if not torch.equal(got, exp):
                ch = int(torch.nonzero(got != exp)[0])
                raise AssertionError(f"{what}: {name} of group {k} differs in {int((got != exp).sum())} channels, first channel {ch}: "
                                     f"got {got[ch].item():.10g} exact {exp[ch].item():.10g}")
    st.check(what + " statistics", used=slots * 2 * c)


# ---------------------------------------------------------------------------------------------------------------------
# runners
# ---------------------------------------------------------------------------------------------------------------------
def run_down(G, prec, dims, x, w, stats=False, group=0, wp=None):
    n, hb, cb, cs = dims
    oh = hb // 2
    out = Guarded(n * oh * oh * cs, DT[prec])
    st = slots = None
    if stats:
        st, slots = Guarded(G.lib.jck_stats_floats(n * oh * oh, cs, 1), torch.float32), ctypes.c_int(-1)
    xd = nhwc(x, DT[prec])
    wp = pack_down(G, w, prec) if wp is None else wp
    a = (prec, xd, wp, out.t, st.t if stats else None, ctypes.byref(slots) if stats else None, n, hb, hb, cb, cs)
    if group:
        G.lib.jck_conv_down_grouped(*a, group, G.cur_stream())
    else:
        G.lib.jck_conv_down(*a, G.cur_stream())
    torch.cuda.synchronize()
    return out, st, slots.value if stats else 0


def run_up(G, prec, dims, x, w, stats=False, group=0, tanh=False):
    n, hs, cs, cb = dims
    cbp = G.lib.jck_pad_chan(cb)
    out = Guarded(n * 4 * hs * hs * cbp, DT[prec])
    st = slots = None
    if stats:
        st, slots = Guarded(G.lib.jck_stats_floats(n * 4 * hs * hs, cbp, 1), torch.float32), ctypes.c_int(-1)
    xd, wp = nhwc(x, DT[prec]), pack_up(G, w, prec)
    sa = (st.t if stats else None, ctypes.byref(slots) if stats else None)
    if group:
        G.lib.jck_conv_up_grouped(prec, xd, wp, out.t, *sa, n, hs, hs, cs, cb, group, G.cur_stream())
    else:
        G.lib.jck_conv_up(prec, xd, wp, out.t, *sa, 1 if tanh else 0, n, hs, hs, cs, cb, G.cur_stream())
    torch.cuda.synchronize()
    return out, st, slots.value if stats else 0


def ref_nhwc(ref, prec, cpad=None):
    """the reference in the layout and storage type of the output: fp32 as it is, bf16 by round-to-nearest-even"""
    return nhwc(ref, torch.float32, cpad).to(DT[prec])


class tuned:
    def __init__(self, G, knob):
        self.G, self.knob = G, knob

    def __enter__(self):
        if self.knob:
            self.G.lib.jck_tune(self.knob.encode(), 0)

    def __exit__(self, *a):
        if self.knob:                 # back to the default: 1, or the JCK_<KEY> preset the library read at load time
            self.G.lib.jck_tune(self.knob.encode(), int(os.environ.get("JCK_" + self.knob.upper(), 1)))


# ---------------------------------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case,prec", items(("down", "up")))
def test_conv_exact(G, case, prec):
    op, dims, opt, kern = case
    stats, group, tanh = bool(opt.get("stats")), opt.get("group", 0), bool(opt.get("tanh"))
    x, w, ref = conv_data(op, dims, stats, group, "tanh" if tanh else None)
    what = f"{case_id(case)} {PREC_NAME[prec]}"
    c_real = dims[3]
    cpad = G.lib.jck_pad_chan(c_real) if op == "up" else c_real
    with tuned(G, opt.get("tune")):
        out, st, slots = (run_down(G, prec, dims, x, w, stats, group) if op == "down" else run_up(G, prec, dims, x, w, stats, group, tanh))
    ran(G, kern[prec], what)
    out.check(what)
    got = out.t.view(ref.shape[0], ref.shape[2], ref.shape[3], cpad)
    if tanh:
        # the one inexact op: the argument is an exact integer in -4..4, what remains is the tanh evaluation and one rounding
        exp = torch.tanh(ref.double())
        g64 = G.from_nhwc(got, c_real).double()
        if prec == 0:
            err = ((g64 - exp).abs() - 2.0 ** -8 * exp.abs()).max().item()
            assert err <= 0, f"{what}: tanh output more than one bf16 ulp (2^-8 relative) off, by {err:.3e}"
        else:
            G.check(g64, exp, max(G.TOL[1], 1e-6), what)
        if cpad != c_real:
            assert int((got[..., c_real:].contiguous().view(IDT[out.esz]) != 0).sum()) == 0, f"{what}: padding channel must be exactly 0"
        return
    expect_equal(got, ref_nhwc(ref, prec, cpad), what, "(n, oy, ox, c)", kern[prec], op, dims)
    if stats:
        check_stats(st, slots, cpad, c_real, ref, (dims[0] // group) if group else 1, what)


@functools.lru_cache(maxsize=1)
def wgrad_data(dims):
    n, hb, cb, cs = dims
    oh = hb // 2
    seed = seed_of("wgrad", dims)
    ds, db = pair_density(n * oh * oh)
    big, small = ternary((n, cb, hb, hb), db, 3, seed), ternary((n, cs, oh, oh), ds, 3, seed + 1)

    def dw(b, s):
        w = torch.zeros(cs, cb, 4, 4, requires_grad=True)
        (F.conv2d(b, w, None, 2, 1) * s).sum().backward()
        return w.grad
    ref, bound = dw(big, small), dw(big.abs(), small.abs()).max()
    conditions(ref, bound, f"wgrad{dims}")
    init = ternary((cs, cb, 4, 4), 1.0, 3, seed + 2)           # accumulate = 1 starts from integers: the sum stays exact
    return big, small, ref, init


@gpu
@pytest.mark.parametrize("case,prec", items(("wgrad",)))
def test_conv_wgrad_exact(G, case, prec):
    op, dims, opt, kern = case
    n, hb, cb, cs = dims
    big, small, ref, init = wgrad_data(dims)
    what = f"{case_id(case)} {PREC_NAME[prec]}"
    sd, bd = nhwc(small, DT[prec]), nhwc(big, DT[prec])
    ws_bytes = G.lib.jck_conv_wgrad_ws_bytes(n, hb, hb, cb, cs)
    with tuned(G, opt.get("tune")):
        for acc in (0, 1):
            ws = Guarded(ws_bytes // 4, torch.float32)
            grad = Guarded(ref.numel(), torch.float32, init if acc else None)
            G.lib.jck_conv_wgrad(prec, sd, bd, ws.t, ws_bytes, grad.t, acc, n, hb, hb, cb, cs, G.cur_stream())
            torch.cuda.synchronize()
            ran(G, kern[prec], what)
            ws.check(what + " workspace")
            grad.check(what)
            expect_equal(grad.t.view(ref.shape), (ref + init if acc else ref).cuda(), f"{what} accumulate={acc}", "(co, ci, kh, kw)",
                         kern[prec], "wgrad", dims)


@functools.lru_cache(maxsize=1)
def g1_data(dims):
    b, ci, cip, co = dims
    seed = seed_of("g1", dims)
    z = ternary((b, ci, 1, 1), 1.0, 3, seed)
    w = fixed_count(co * 16, ci, 14, seed + 1).view(co, 16, ci).permute(2, 0, 1).reshape(ci, co, 4, 4).contiguous()
    ref, bound = F.conv_transpose2d(z, w, None, 1, 0), F.conv_transpose2d(z.abs(), w.abs(), None, 1, 0).max()
    conditions(ref, bound, f"g1{dims}", (0, 2, 3))
    sd, sb = pair_density(b)
    zz, dy = ternary((b, ci), sd, 3, seed + 2), ternary((b, co, 4, 4), sb, 3, seed + 3)
    gref = torch.einsum("bi,bokl->iokl", zz.double(), dy.double())
    conditions(gref.float(), torch.einsum("bi,bokl->iokl", zz.abs().double(), dy.abs().double()).max(), f"g1w{dims}")
    return z, w, ref, zz, dy, gref.float()


@gpu
@pytest.mark.parametrize("case,prec", items(("g1", "g1w")))
def test_g1_exact(G, case, prec):
    op, dims, opt, kern = case
    b, ci, cip, co = dims
    z, w, ref, zz, dy, gref = g1_data(dims)
    what = f"{case_id(case)} {PREC_NAME[prec]}"

    def pad(v):
        zp = torch.zeros(b, cip)
        zp[:, :ci] = v.view(b, ci)
        return zp.to(DT[prec]).cuda()
    if op == "g1":
        wp = torch.empty(16 * co * cip, dtype=DT[prec], device="cuda")
        G.lib.jck_pack_g1(prec, w.cuda(), ci, co, cip, wp, G.cur_stream())
        out = Guarded(b * 16 * co, DT[prec])
        st, slots = Guarded(G.lib.jck_stats_floats(b * 16, co, 16), torch.float32), ctypes.c_int(-1)
        G.lib.jck_g1_fwd(prec, pad(z), wp, out.t, st.t, ctypes.byref(slots), b, cip, co, G.cur_stream())
        torch.cuda.synchronize()
        ran(G, kern[prec], what)
        out.check(what)
        expect_equal(out.t.view(b, 4, 4, co), ref_nhwc(ref, prec), what, "(b, kh, kw, co)", kern[prec], "g1", dims)
        check_stats(st, slots.value, co, co, ref, 1, what)
        return
    ws_bytes = G.lib.jck_g1_wgrad_ws_bytes(b, cip, co)
    init = ternary((ci, co, 4, 4), 1.0, 3, 77)
    with tuned(G, opt.get("tune")):
        for acc in (0, 1):
            ws, grad = Guarded(ws_bytes // 4, torch.float32), Guarded(gref.numel(), torch.float32, init if acc else None)
            G.lib.jck_g1_wgrad(prec, pad(zz), nhwc(dy, DT[prec]), ws.t, ws_bytes, grad.t, acc, b, ci, cip, co, G.cur_stream())
            torch.cuda.synchronize()
            ran(G, kern[prec], what)
            ws.check(what + " workspace")
            grad.check(what)
            expect_equal(grad.t.view(gref.shape), (gref + init if acc else gref).cuda(), f"{what} accumulate={acc}", "(ci, co, kh, kw)", kern[prec], "g1w", dims)


@functools.lru_cache(maxsize=1)
def lin_data(dims):
    b, k, kp, n = dims[:4]
    seed = seed_of("lin", dims[:4])
    x = ternary((b, k), 0.25 if k >= 256 else 1.0, 3, seed)
    w = fixed_count(n, k, round(64 / ((0.25 if k >= 256 else 1.0) * 14 / 3)), seed + 1)
    ref = x @ w.t()
    conditions(ref, (x.abs() @ w.abs().t()).max(), f"lin{dims}")
    return x, w, ref


@gpu
@pytest.mark.parametrize("case,prec", items(("lin",)))
def test_linear_fwd_exact(G, case, prec):
    """split-K: every fp32 slab equals the product over its own k-range, and their sum the whole; ksplit = 1: bias added, columns
    N .. NStore hold the bias alone (their weight rows are the packing's zero rows)"""
    op, dims, opt, kern = case
    b, k, kp, n, nstore, ks, bias = dims
    x, w, ref = lin_data(dims)
    what = f"{case_id(case)} {PREC_NAME[prec]}"
    rows = G.lib.jck_pad_rows(n)
    xp = torch.zeros(b, kp)
    xp[:, :k] = x
    wp = torch.empty(rows * kp, dtype=DT[prec], device="cuda")
    G.lib.jck_pack_linear(prec, w.cuda(), n, k, rows, kp, 0, 0, 0, wp, G.cur_stream())
    bv = ternary((nstore,), 1.0, 3, 5) if bias else None
    out = Guarded(ks * b * nstore, torch.float32 if ks > 1 else DT[prec])
    with tuned(G, opt.get("tune")):
        G.lib.jck_linear_fwd(prec, xp.to(DT[prec]).cuda(), wp, bv.cuda() if bias else None, out.t, b, kp, n, nstore, ks, G.cur_stream())
        torch.cuda.synchronize()
    ran(G, kern[prec], what)
    out.check(what)
    if ks > 1:
        step = kp // ks
        wpad = torch.zeros(n, kp)
        wpad[:, :k] = w
        exp = torch.stack([xp[:, i * step:(i + 1) * step] @ wpad[:, i * step:(i + 1) * step].t() for i in range(ks)])
        got = out.t.view(ks, b, nstore)
        expect_equal(got[..., :n].contiguous(), exp.cuda(), what + " slabs", "(slab, row, column)", kern[prec], "lin", dims)
        expect_equal(got.sum(0)[:, :n].contiguous(), ref.cuda(), what + " sum of the slabs", "(row, column)", kern[prec], "lin", dims)
        return
    exp = torch.zeros(b, nstore)
    exp[:, :n] = ref
    if bias:
        exp += bv
    expect_equal(out.t.view(b, nstore), exp.to(DT[prec]).cuda(), what, "(row, column)", kern[prec], "lin", dims)


@gpu
@pytest.mark.parametrize("case,prec", items(("linw",)))
def test_linear_wgrad_exact(G, case, prec):
    op, dims, opt, kern = case
    b, n, k, kp, ldgy, pc, phw = dims
    what = f"{case_id(case)} {PREC_NAME[prec]}"
    seed = seed_of("linw", dims)
    sd, sb = pair_density(b)
    gy, x = ternary((b, n), sd, 3, seed), ternary((b, k), sb, 3, seed + 1)        # x in the library's column order
    ref = gy.t() @ x                                                            # [N][K], our column order
    conditions(ref, (gy.abs().t() @ x.abs()).max(), what)
    gyp = torch.full((b, ldgy), 1e6)                                            # columns past N: never read
    gyp[:, :n] = gy
    xp = torch.zeros(b, kp)
    xp[:, :k] = x
    ws_bytes = G.lib.jck_linear_wgrad_ws_bytes(b, kp, n)
    init = ternary((n, kp), 1.0, 3, seed + 2)

    def unperm(m):                                                              # ours [hw][c] -> torch's [c][hw] on the first pc * phw columns
        m = m.clone()
        if pc:
            m[:, :pc * phw] = m[:, :pc * phw].view(n, phw, pc).transpose(1, 2).reshape(n, pc * phw)
        return m
    with tuned(G, opt.get("tune")):
        for acc in (0, 1):
            ws, gp = Guarded(ws_bytes // 4, torch.float32), Guarded(n * kp, torch.float32, init if acc else None)
            G.lib.jck_linear_wgrad(prec, gyp.to(DT[prec]).cuda(), ldgy, xp.to(DT[prec]).cuda(), kp, ws.t, ws_bytes, gp.t, acc, b, n, G.cur_stream())
            torch.cuda.synchronize()
            ran(G, kern[prec], what)
            ws.check(what + " workspace")
            gp.check(what)
            exp = torch.zeros(n, kp)
            exp[:, :k] = ref
            expect_equal(gp.t.view(n, kp), (exp + init if acc else exp).cuda(), f"{what} accumulate={acc}", "(n, k)", kern[prec], "linw", dims)
            gw = Guarded(n * k, torch.float32, init[:, :k].contiguous() if acc else None)
            G.lib.jck_unperm_linear_grad(gp.t, n, k, kp, pc, phw, gw.t, acc, G.cur_stream())
            torch.cuda.synchronize()
            gw.check(what + " unperm")
            e2 = unperm((ref + init[:, :k]) if acc else ref) + (init[:, :k] if acc else 0)    # gp holds init + ref when accumulating
            expect_equal(gw.t.view(n, k), e2.cuda(), f"{what} unperm accumulate={acc}", "(n, k)")


@gpu
@pytest.mark.parametrize("prec", [0, 1, 2])
@pytest.mark.parametrize("b,c", [(16, 512), (21, 512),              # small and ragged
                                 (256, 512), (128, 1024),          # d_head_backward, per-pass: jck_head_bwd_conv over B rows (csrc/engine.hip)
                                 (768, 512), (384, 1024)])         # d_batched_pass: head_bwd_conv2 over 2B loss rows + B penalty rows
def test_head_bwd_exact(G, prec, b, c):
    """jck_head_bwd (dgrad + packed weight gradient, both accumulate modes), jck_head_bwd_conv and jck_head_bwd_conv2 with ds drawn
    from signed powers of two (2^-2 .. 2^2): ds * wp and every partial sum of ds * a4 are exact (multiples of 1/4 below 2^24 / 4)"""
    k = 16 * c
    g = _gen(b + c)
    ds = (2.0 ** torch.randint(-2, 3, (b,), generator=g).float()) * (torch.randint(0, 2, (b,), generator=g) * 2 - 1).float()
    w = ternary((1, c, 4, 4), 1.0, 3, 11)
    a4 = ternary((b, c, 4, 4), 1.0, 3, 12)
    assert float((ds.abs().view(b, 1, 1, 1) * a4.abs()).sum(0).max()) * 4 < LIM
    wp = torch.empty(k, device="cuda")
    G.lib.jck_pack_head(w.cuda(), c, wp, G.cur_stream())
    wpk = w[0].permute(1, 2, 0).reshape(k)                                     # packed (kh, kw, c) order
    a4d, dsd = nhwc(a4, DT[prec]), ds.cuda()
    a4k = a4.permute(0, 2, 3, 1).reshape(b, k)
    ga_ref = (ds.view(b, 1) * wpk.view(1, k)).to(DT[prec]).cuda()
    dwp_ref = (ds.view(b, 1).double() * a4k.double()).sum(0).float()
    gw_ref = dwp_ref.view(4, 4, c).permute(2, 0, 1).reshape(1, c, 4, 4)
    init = ternary((k,), 1.0, 3, 13)
    what = f"head b={b} c={c} {PREC_NAME[prec]}"
    hws = Guarded(G.lib.jck_head_bwd_ws_floats(k), torch.float32)
    for acc in (0, 1):
        ga, dwp = Guarded(b * k, DT[prec]), Guarded(k, torch.float32, init if acc else None)
        G.lib.jck_head_bwd(prec, dsd, wp, a4d, b, k, ga.t, dwp.t, acc, hws.t, G.cur_stream())
        torch.cuda.synchronize()
        ga.check(what), dwp.check(what), hws.check(what + " workspace")
        expect_equal(ga.t.view(b, k), ga_ref, what + " head_bwd dgrad", "(n, k)")
        expect_equal(dwp.t, (dwp_ref + init if acc else dwp_ref).cuda(), f"{what} head_bwd dwp accumulate={acc}", "(k,)")
    gi = init.view(1, c, 4, 4)
    ga, gw = Guarded(b * k, DT[prec]), Guarded(k, torch.float32, gi)
    G.lib.jck_head_bwd_conv(prec, dsd, wp, a4d, b, c, ga.t, gw.t, hws.t, G.cur_stream())
    torch.cuda.synchronize()
    ga.check(what), gw.check(what), hws.check(what + " workspace")
    expect_equal(ga.t.view(b, k), ga_ref, what + " head_bwd_conv dgrad", "(n, k)")
    expect_equal(gw.t.view(1, c, 4, 4), (gw_ref + gi).cuda(), what + " head_bwd_conv grad", "(0, c, kh, kw)")
    b1 = b - b // 3                                                             # loss rows, then rows that only get their input gradient
    ga, gw = Guarded(b * k, DT[prec]), Guarded(k, torch.float32, gi)
    G.lib.jck_head_bwd_conv2(prec, dsd, wp, a4d, b1, b - b1, c, ga.t, gw.t, hws.t, G.cur_stream())
    torch.cuda.synchronize()
    ga.check(what), gw.check(what), hws.check(what + " workspace")
    expect_equal(ga.t.view(b, k), ga_ref, what + " head_bwd_conv2 dgrad", "(n, k)")
    g1 = (ds[:b1].view(b1, 1).double() * a4k[:b1].double()).sum(0).float().view(4, 4, c).permute(2, 0, 1).reshape(1, c, 4, 4)
    expect_equal(gw.t.view(1, c, 4, 4), (g1 + gi).cuda(), what + " head_bwd_conv2 grad", "(0, c, kh, kw)")


@gpu
@pytest.mark.parametrize("prec", [0, 1, 2])
@pytest.mark.parametrize("b", [256, 512, 768, 21])
def test_head_bwd_linear2_exact(G, prec, b):
    """CGAN's Linear(256,1) backward as the engine's d_head_backward issues it (csrc/engine.hip): jck_head_bwd with K = L1_OUT = 256
    on the dropped-out hidden rows, accumulate = 1, and exactly ONE of the two outputs - the input gradient alone over B or 3B rows,
    the weight gradient alone over B or 2B rows.  K = 256 is a single partial column block of the weight-gradient kernel."""
    k = 256
    g = _gen(900 + b)
    ds = (2.0 ** torch.randint(-2, 3, (b,), generator=g).float()) * (torch.randint(0, 2, (b,), generator=g) * 2 - 1).float()
    w2, hd = ternary((k,), 1.0, 3, 21), ternary((b, k), 1.0, 3, 22)
    assert float((ds.abs().view(b, 1) * hd.abs()).sum(0).max()) * 4 < LIM
    init = ternary((k,), 1.0, 3, 23)
    what = f"linear2 head b={b} {PREC_NAME[prec]}"
    w2d, hdd, dsd = w2.cuda(), hd.to(DT[prec]).cuda(), ds.cuda()
    hws = Guarded(G.lib.jck_head_bwd_ws_floats(k), torch.float32)
    ga = Guarded(b * k, DT[prec])
    G.lib.jck_head_bwd(prec, dsd, w2d, hdd, b, k, ga.t, None, 1, hws.t, G.cur_stream())          # input gradient only
    torch.cuda.synchronize()
    ga.check(what), hws.check(what + " workspace", used=0)
    expect_equal(ga.t.view(b, k), (ds.view(b, 1) * w2.view(1, k)).to(DT[prec]).cuda(), what + " dgrad only", "(n, k)")
    dw = Guarded(k, torch.float32, init)
    G.lib.jck_head_bwd(prec, dsd, w2d, hdd, b, k, None, dw.t, 1, hws.t, G.cur_stream())           # weight gradient only, accumulated
    torch.cuda.synchronize()
    dw.check(what), hws.check(what + " workspace")
    expect_equal(dw.t, ((ds.view(b, 1).double() * hd.double()).sum(0).float() + init).cuda(), what + " dwp only, accumulate=1", "(k,)")


# the rounding cases: bf16 stores of exact fp32 accumulators in (256, 4096) must round to nearest even
@gpu
@pytest.mark.parametrize("op,dims,kernel", [("down", (4, 16, 64, 128), "igemm_dma_persist<128,64,4>"),
                                            ("up", (4, 8, 512, 128), "igemm_dma_persist<128,64,4>")])
def test_bf16_store_rounds_to_nearest_even(G, op, dims, kernel):
    x, w, ref = conv_data(op, dims, False, 0, "round")
    r = ref.double().abs()
    ulp = 2.0 ** (torch.floor(torch.log2(r.clamp(min=1))) - 7)
    ties = int(((r >= 256) & (torch.remainder(r, ulp) == ulp / 2)).sum())
    print(f"{op}{dims}: {ties} exact ties of {ref.numel()} outputs, max |y| {int(r.max())}")
    assert ties >= 100, f"only {ties} ties: the case would prove nothing about ties"
    out, _, _ = run_down(G, 0, dims, x, w) if op == "down" else run_up(G, 0, dims, x, w)
    ran(G, kernel, f"rounding {op}")
    out.check(f"rounding {op}")
    expect_equal(out.t.view(ref.shape[0], ref.shape[2], ref.shape[3], ref.shape[1]), ref_nhwc(ref, 0), f"rounding {op}{dims} ({ties} ties)",
                 "(n, oy, ox, c)", kernel, op, dims)


# impulse cases: +1 on one input element / one weight element; the output difference is the weight slice / the input patch at
# exactly the outputs that read it and 0 elsewhere.  The expected difference is built tap by tap, not by a convolution.
def _delta(op, dims, x, w, kind, at):
    n, h, c_in, c_out = dims
    ho = h // 2 if op == "down" else 2 * h
    d = torch.zeros(n, c_out, ho, ho)
    for kh in range(4):
        for kw in range(4):
            if op == "down":            # out[n, co, oy, ox] += x[n, ci, 2 oy - 1 + kh, 2 ox - 1 + kw] * w[co, ci, kh, kw]
                if kind == "x":
                    ni, ci, y, xx = at
                    if (y + 1 - kh) % 2 == 0 and (xx + 1 - kw) % 2 == 0 and 0 <= (y + 1 - kh) // 2 < ho and 0 <= (xx + 1 - kw) // 2 < ho:
                        d[ni, :, (y + 1 - kh) // 2, (xx + 1 - kw) // 2] += w[:, ci, kh, kw]
                else:
                    co, ci, a, b = at
                    if (a, b) == (kh, kw):
                        xp = F.pad(x[:, ci], (1, 1, 1, 1))
                        d[:, co] += xp[:, kh:kh + 2 * ho:2, kw:kw + 2 * ho:2]
            else:                       # out[n, cb, 2 iy - 1 + kh, 2 ix - 1 + kw] += x[n, cs, iy, ix] * w[cs, cb, kh, kw]
                if kind == "x":
                    ni, ci, y, xx = at
                    oy, ox = 2 * y - 1 + kh, 2 * xx - 1 + kw
                    if 0 <= oy < ho and 0 <= ox < ho:
                        d[ni, :, oy, ox] += w[ci, :, kh, kw]
                else:
                    ci, co, a, b = at
                    if (a, b) == (kh, kw):
                        for iy in range(h):
                            oy = 2 * iy - 1 + kh
                            if 0 <= oy < ho:
                                ix = torch.arange(h)
                                ox = 2 * ix - 1 + kw
                                ok = (ox >= 0) & (ox < ho)
                                d[:, co, oy, ox[ok]] += x[:, ci, iy, ix[ok]]
    return d


_KD = ("igemm_dma_persist<128,64,4>", "igemm<f32,128,64>", "igemm<bf16x3,128,64>")
_KU = ("igemm_dma_persist<64,128,4>", "igemm<f32,64,128>", "igemm<bf16x3,64,128>")
IMPULSES = [("down", (5, 16, 64, 128), "x", (0, 0, 0, 0), _KD),          # an image corner
            ("down", (5, 16, 64, 128), "x", (2, 37, 0, 15), _KD),        # a tile seam: image 2 starts pixel tile 1 of 128 pixels / tile 2 of 64
            ("down", (5, 16, 64, 128), "x", (4, 63, 15, 15), _KD),       # the last element of the last image
            ("down", (5, 16, 64, 128), "w", (17, 3, 2, 1), _KD),
            ("up", (5, 8, 128, 64), "x", (4, 127, 7, 7), _KU),
            ("up", (5, 8, 128, 64), "w", (3, 17, 3, 0), _KU)]


@gpu
@pytest.mark.parametrize("prec", [0, 1, 2])
@pytest.mark.parametrize("op,dims,kind,at,kern", IMPULSES)
def test_impulse(G, prec, op, dims, kind, at, kern):
    x, w, ref = conv_data(op, dims, False, 0, "impulse")
    x2, w2 = x.clone(), w.clone()
    (x2 if kind == "x" else w2)[at] += 1
    d = _delta(op, dims, x, w, kind, at)
    nz = int((d != 0).sum())
    assert nz > 0 and (kind == "w" or nz == int((d.abs().sum(1) != 0).sum()) * dims[3]), "an input impulse must answer in every channel"
    assert float((ref + d).abs().max()) <= 256                   # both outputs are exact in bf16: so is their difference
    run = run_down if op == "down" else run_up
    what = f"impulse {op}{dims} {kind}{at} {PREC_NAME[prec]}"
    o1, _, _ = run(G, prec, dims, x, w)
    ran(G, kern[prec], what)
    o2, _, _ = run(G, prec, dims, x2, w2)
    ran(G, kern[prec], what)
    o1.check(what), o2.check(what)
    shape = (ref.shape[0], ref.shape[2], ref.shape[3], ref.shape[1])
    got = o2.t.view(shape).float() - o1.t.view(shape).float()
    expect_equal(got, nhwc(d, torch.float32), what + ": out(perturbed) - out", "(n, oy, ox, c)", kern[prec], op, dims)


def test_every_kernel_has_an_exact_case(G):
    """static: every kernel name the library can report is the target of an exact case in each precision it exists for (built from
    the table, so it holds under -k selection).  Needs the library, not a GPU."""
    names, i = [], 0
    while True:
        s = G.lib.jck_launch_name(i)
        if s is None:
            break
        names.append(s.decode())
        i += 1
    assert len(names) == len(set(names)) and len(names) >= 30
    targets = {k for c in CASES for k in c[3] if k}
    unreachable = {}                    # name -> reason + the engine call site that reaches it; empty: everything is reachable through the C ABI
    missing = sorted(set(names) - targets - set(unreachable))
    unknown = sorted(targets - set(names))
    assert not missing, f"no exact case targets {missing}"
    assert not unknown, f"the table names kernels the library does not have: {unknown}"
    for c in CASES:                      # a name's precision tag agrees with the column it stands in
        for p, k in enumerate(c[3]):
            m = re.match(r"(?:igemm|wgrad)<(bf16x3|bf16|f32),", k or "")
            assert not m or m.group(1) == PREC_NAME[p], f"{case_id(c)}: {k} in the {PREC_NAME[p]} column"
            assert not k or PREC_NAME[p] == "bf16" or not re.match(r"igemm_dma|wgrad_dma|img_", k), f"{case_id(c)}: {k} is a bf16 kernel"
