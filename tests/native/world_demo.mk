# Builds world_demo (the host mirror's assembleWorldMap, host/ndt_feature_graph_gpu.h) against the in-tree libndtgpu.so:
#   make -f world_demo.mk            (tests/test_host_world.py builds the same way; g++ only, no ROS / Eigen / PCL needed)
CXX ?= g++
PKG := $(abspath ../../ndt_feature_graph_amd)
HOST := $(PKG)/host
world_demo: world_demo.cpp $(HOST)/ndt_feature_graph_gpu.h $(HOST)/lslgeneric_gpu.h $(HOST)/ndt_gpu_types.h ../../include/ndtgpu.h $(PKG)/libndtgpu.so
	$(CXX) -O2 -std=c++17 -Wall -Wextra -I$(HOST) world_demo.cpp -o $@ -L$(PKG) -lndtgpu -Wl,-rpath,$(PKG) -Wl,-rpath,/opt/rocm/lib
clean:
	rm -f world_demo
