# How a program that includes the shim is compiled and linked: the one place for tests/cpp/Makefile and oracle/Makefile, which
# set REF (the reference tree) and ROOT (this repository) before they include it.
# -std=c++14, PIRE_NO_CONFIG and -include limits: see REFFLAGS in oracle/Makefile.
OUT      ?= $(ROOT)/oracle/_ref
CXX      ?= g++
SHIMINC  ?= $(ROOT)/include
BINFLAGS := -std=c++14 -O1 -DPIRE_NO_CONFIG -w -include limits -I$(REF) -I$(REF)/pire
REFLINK  := -L$(OUT) -lpire_ref -Wl,-rpath,'$$ORIGIN/..'
HIPLINK  := -L$(ROOT)/pire_amd -lpire_hip -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,'$$ORIGIN/../../../pire_amd' -Wl,-rpath,/opt/rocm/lib
SHIMHDR  := $(SHIMINC)/pire_hip/batch_runner.hpp $(SHIMINC)/pire_hip.h
