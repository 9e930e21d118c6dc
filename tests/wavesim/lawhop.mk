# TEST INFRASTRUCTURE: csrc/tmpc_law.hip's kernel with the hops of its search on the host execution model of hip_sim.hpp, under ASan + UBSan and under MSan.
# `make -f lawhop.mk` in this directory; see Makefile for the toolchain.
CXX = /opt/rocm/lib/llvm/bin/clang++
PKG = ../../robust-tracking-mpc-over-lossy-networks_amd
FLAGS = $(EXTRA) -std=c++20 -g -fno-omit-frame-pointer -DTMPC_HOST_SIM -I. -I$(PKG)/csrc -Wno-unused-function -Wno-unknown-attributes -Wno-psabi
LSRC = lawhop_main.cpp hip_sim.hpp $(PKG)/csrc/tmpc_law.hip $(PKG)/csrc/tmpc_law.hpp $(PKG)/csrc/tmpc_law_wave.hpp $(PKG)/csrc/tmpc_device.hpp $(PKG)/csrc/tmpc_launch.hpp \
       $(PKG)/../include/tmpc.h

all: _build/lawhop_asan _build/lawhop_msan

_build/lawhop_asan: $(LSRC)
	@mkdir -p _build
	$(CXX) $(FLAGS) -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined lawhop_main.cpp -o $@

_build/lawhop_msan: $(LSRC)
	@mkdir -p _build
	$(CXX) $(FLAGS) -O1 -fsanitize=memory -fsanitize-memory-track-origins lawhop_main.cpp -o $@
