# TEST INFRASTRUCTURE: csrc/tmpc_series.hip's reduction kernel on the host execution model of hip_sim.hpp, under ASan + UBSan and under MSan.
# `make -f series.mk` in this directory; see Makefile for the toolchain.
CXX = /opt/rocm/lib/llvm/bin/clang++
PKG = ../../robust-tracking-mpc-over-lossy-networks_amd
FLAGS = $(EXTRA) -std=c++20 -g -fno-omit-frame-pointer -DTMPC_HOST_SIM -I. -I$(PKG)/csrc -Wno-unused-function -Wno-unknown-attributes -Wno-psabi
SSRC = seriessim_main.cpp hip_sim.hpp west_sim.hpp $(PKG)/csrc/tmpc_series.hip $(PKG)/csrc/tmpc_series.hpp $(PKG)/csrc/tmpc_device.hpp \
       $(PKG)/csrc/tmpc_launch.hpp $(PKG)/csrc/tmpc_west.hpp $(PKG)/../include/tmpc.h

all: _build/seriessim_asan _build/seriessim_msan

_build/seriessim_asan: $(SSRC)
	@mkdir -p _build
	$(CXX) $(FLAGS) -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined seriessim_main.cpp -o $@

_build/seriessim_msan: $(SSRC)
	@mkdir -p _build
	$(CXX) $(FLAGS) -O1 -fsanitize=memory -fsanitize-memory-track-origins seriessim_main.cpp -o $@
