# TEST INFRASTRUCTURE: csrc/tmpc_law.hip's kernel on the host execution model of hip_sim.hpp, under ASan + UBSan and under MSan.
# `make -f law.mk` in this directory; see Makefile for the toolchain.
CXX = /opt/rocm/lib/llvm/bin/clang++
PKG = ../../robust-tracking-mpc-over-lossy-networks_amd
FLAGS = $(EXTRA) -std=c++20 -g -fno-omit-frame-pointer -DTMPC_HOST_SIM -I. -I$(PKG)/csrc -Wno-unused-function -Wno-unknown-attributes -Wno-psabi
LSRC = lawsim_main.cpp hip_sim.hpp $(PKG)/csrc/tmpc_law.hip $(PKG)/csrc/tmpc_law.hpp $(PKG)/csrc/tmpc_device.hpp $(PKG)/csrc/tmpc_launch.hpp \
       $(PKG)/../include/tmpc.h

all: _build/lawsim_asan _build/lawsim_msan

_build/lawsim_asan: $(LSRC)
	@mkdir -p _build
	$(CXX) $(FLAGS) -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined lawsim_main.cpp -o $@

_build/lawsim_msan: $(LSRC)
	@mkdir -p _build
	$(CXX) $(FLAGS) -O1 -fsanitize=memory -fsanitize-memory-track-origins lawsim_main.cpp -o $@
