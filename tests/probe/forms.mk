# libmacm_forms_probe.so for tests/test_gpu_f64_forms.py (built by __graft_entry__.py build():
# make -C tests/probe -f forms.mk): the written-out f64 division of csrc/macm_math.h beside the
# compiler's `/` (f64_forms_probe.hip), gfx950. HIPCC, ARCH and HIPFLAGS are the product's, from
# gym-macm_amd/hipflags.mk, as in the Makefile beside this file and for the same reason: the probe
# has to test the code the product compiles.
PKG := ../../gym-macm_amd
include $(PKG)/hipflags.mk

all: libmacm_forms_probe.so

libmacm_forms_probe.so: f64_forms_probe.hip $(PKG)/csrc/macm_math.h $(PKG)/csrc/trig_fix.inc $(PKG)/hipflags.mk
	$(HIPCC) $(HIPFLAGS) -I $(PKG)/csrc -shared -o $@ f64_forms_probe.hip

clean:
	rm -f libmacm_forms_probe.so
.PHONY: all clean
