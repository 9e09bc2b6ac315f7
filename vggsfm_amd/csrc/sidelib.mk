# The rules of a side library: a gfx950 shared object of its own in-tree, beside libvggsfm_amd.so (the entries of each are a
# closed, counted set).  Included by <dir>/Makefile, which sets OUT, SRC and HEADER.  Every side library is one parity file:
# built with -ffp-contract=off, the unfused arithmetic that its tests/*_cases.py restates.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
COMMON = --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -munsafe-fp-atomics -Wall -Wno-unused-function
# the library's own header and the headers the side libraries share
HDRS = $(HEADER) ../common.hpp ../crosslane.hpp ../scan.hpp ../jacobi.hpp $(wildcard ../mvs/*.hpp) $(wildcard ../nn/*.hpp)
# (OBJDIR and EXTRA: a measurement build of the same recipe with other constants, e.g. scripts/time_icp.py)
OBJDIR ?= _obj
EXTRA ?=
OBJ = $(OBJDIR)/$(basename $(SRC)).o

all: $(OUT)

$(OBJ): $(SRC) $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(COMMON) $(EXTRA) -ffp-contract=off -c $< -o $@

$(OUT): $(OBJ)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(OBJ)

clean:
	rm -rf $(OBJDIR) $(OUT)
