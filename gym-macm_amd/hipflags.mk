# The compiler and flags every HIP source of the product is built with, in a fragment of its own so
# that tests/probe/Makefile builds its kernels around the product's device functions with the same
# ones (include, never retype: a probe built with other flags tests other code).
# -ffp-contract=off keeps every float op separately rounded, as in Box2D's
# SSE2 build and the reference's numpy double math (see csrc/flock_common.hpp).
# -fno-slp-vectorize: the compiler's pairing of scalar f32 ops into v_pk_* puts hazard nops on
# the serial contact-solver chains (C5 -3.6%, C4 -0.9%, M neutral; profiles/r01/ab2 s20); the
# sweep's packed ops are explicit vector types and stay packed.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
HIPFLAGS ?= --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -ffp-contract=off -fno-slp-vectorize -Wall -Wno-unused-result
