# TEST INFRASTRUCTURE: the fused closed loop through the explicit law (closed_loop_law: csrc/tmpc_kernels.hip with FUSED = 3) with the hops of its search on the host
# execution model of hip_sim.hpp, under ASan + UBSan and under MSan; the bench shape only.  `make -f lawloophop.mk` in this directory; see
# Makefile for the toolchain.  TMPC_SIM_LAW_LOOP is what puts the kernel into a host-model binary: the binaries of Makefile do not hold it.
CXX = /opt/rocm/lib/llvm/bin/clang++
PKG = ../../robust-tracking-mpc-over-lossy-networks_amd
FLAGS = $(EXTRA) -std=c++20 -g -fno-omit-frame-pointer -DTMPC_HOST_SIM -DTMPC_SIM_LAW_LOOP -DTMPC_ONLY_BENCH -I. -I$(PKG)/csrc -Wno-unused-function -Wno-unknown-attributes -Wno-psabi
LSRC = lawloophop_main.cpp hip_sim.hpp $(PKG)/csrc/tmpc_kernels.hip $(PKG)/csrc/tmpc_wave.hpp $(PKG)/csrc/tmpc_device.hpp $(PKG)/csrc/tmpc_launch.hpp \
       $(PKG)/csrc/tmpc_mc_step.hpp $(PKG)/csrc/tmpc_law.hpp $(PKG)/csrc/tmpc_law_wave.hpp $(PKG)/../include/tmpc.h

all: _build/lawloophop_asan _build/lawloophop_msan

_build/lawloophop_asan: $(LSRC)
	@mkdir -p _build
	$(CXX) $(FLAGS) -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined lawloophop_main.cpp -o $@

_build/lawloophop_msan: $(LSRC)
	@mkdir -p _build
	$(CXX) $(FLAGS) -O1 -fsanitize=memory -fsanitize-memory-track-origins lawloophop_main.cpp -o $@
