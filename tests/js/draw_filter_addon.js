'use strict';
/* The N-API shim's drawListFilteredDevice and drawFilterFactors on the CPU (driven by tests/test_draw_filter_cpu.py):
 *     node tests/js/draw_filter_addon.js <addon.node built from csrc/ht_napi.cc + tests/js/abi_stub.cc + draw_list_stub.cc + draw_filter_stub.cc>
 * Successful calls (what reaches the C ABI is in the stubs' logs) and every malformed call (the message each one throws is printed).  ONE
 * device buffer holds all sources, so that the stub can log plane pointers relative to the first entry's.  Prints one JSON line. */
const A = require(process.argv[2]);
const out = { kinds: [typeof A.drawListFilteredDevice, typeof A.drawFilterFactors, typeof A.drawListDevice], thrown: [] };
const c = A.createContext({ cascade: new Uint8Array(64), interval: 5, device: 0 });
A.setGeometry(c, 40, 30, 4, null);
const fb = 40 * 30 * 4;
const src = A.deviceAlloc(c, 100000), dst = A.deviceAlloc(c, 4 * fb + 100), small = A.deviceAlloc(c, 16);
const rgba = { dev: src, offset: 0, width: 7, height: 5, format: A.DRAW_RGBA, matrix: 0, rect: null };
const nv12 = { dev: src, offset: 1001, width: 23, height: 23, format: A.YUV_NV12, matrix: 1, rect: Int32Array.from([1, 1, 21, 21]) };
const i420 = { dev: src, offset: 4000, width: 97, height: 81, format: A.YUV_I420, matrix: 3, rect: undefined };
const tail = { dev: src, offset: 100000 - 6, width: 2, height: 2, format: A.YUV_I420 };
A.drawListFilteredDevice(c, [rgba, nv12, i420, tail], 8, dst, 0);                    /* the 5-argument form: packed frames at offset 0, no wait */
A.drawListFilteredDevice(c, [nv12, { dev: src, width: 7, height: 5, format: A.DRAW_RGBA, offset: undefined }], 3, dst, fb + 48, 4, true);  /* stride, offset, wait */
A.drawListFilteredDevice(c, [i420], 1, null, 0);                                      /* the bind form */
A.drawListDevice(c, [rgba, nv12], dst, 0);                                            /* the plain call goes on reaching ITS function */
const f = A.drawFilterFactors(Int32Array.from([1920, 1080, 7, 5]), 320, 240, 8);
out.factors = Array.from(f); out.factorsKind = f.constructor.name;
out.noFactors = Array.from(A.drawFilterFactors(new Int32Array(0), 1, 1, 1));
function bad(what, fn) { try { fn(); out.thrown.push([what, null]); } catch (e) { out.thrown.push([what, e.constructor.name + ': ' + e.message]); } }
bad('too few arguments', function () { A.drawListFilteredDevice(c, [rgba], 8, dst); });
bad('the plain arguments', function () { A.drawListFilteredDevice(c, [rgba], dst, 0); });
bad('no context', function () { A.drawListFilteredDevice(dst, [rgba], 8, dst, 0); });
bad('entries no array', function () { A.drawListFilteredDevice(c, rgba, 8, dst, 0); });
bad('no entries', function () { A.drawListFilteredDevice(c, [], 8, dst, 0); });
bad('maxFactor a string', function () { A.drawListFilteredDevice(c, [rgba], 'eight', dst, 0); });
bad('maxFactor 0', function () { A.drawListFilteredDevice(c, [rgba], 0, dst, 0); });
bad('maxFactor 9', function () { A.drawListFilteredDevice(c, [rgba], 9, dst, 0); });
bad('maxFactor -1', function () { A.drawListFilteredDevice(c, [rgba], -1, dst, 0); });
bad('entry no object', function () { A.drawListFilteredDevice(c, [rgba, 5], 8, dst, 0); });
bad('entry without dev', function () { A.drawListFilteredDevice(c, [{ width: 7, height: 5, format: A.DRAW_RGBA }], 8, dst, 0); });
bad('width a string', function () { A.drawListFilteredDevice(c, [Object.assign({}, rgba, { width: 'wide' })], 8, dst, 0); });
bad('rect a plain array', function () { A.drawListFilteredDevice(c, [Object.assign({}, rgba, { rect: [0, 0, 4, 4] })], 8, dst, 0); });
bad('frame beyond its buffer', function () { A.drawListFilteredDevice(c, [Object.assign({}, tail, { offset: 100000 - 5 })], 8, dst, 0); });
bad('RGBA frame beyond its buffer', function () { A.drawListFilteredDevice(c, [Object.assign({}, rgba, { dev: small })], 8, dst, 0); });
bad('destination too small', function () { A.drawListFilteredDevice(c, [rgba, rgba, rgba, rgba, rgba], 8, dst, 0); });
bad('destination offset beyond', function () { A.drawListFilteredDevice(c, [rgba, rgba, rgba, rgba], 8, dst, 0, 104); });
bad('destination stride beyond', function () { A.drawListFilteredDevice(c, [rgba, rgba], 8, dst, 4 * fb); });
bad('dst a context', function () { A.drawListFilteredDevice(c, [rgba], 8, c, 0); });
bad('stride a string', function () { A.drawListFilteredDevice(c, [rgba], 8, dst, 'packed'); });
bad('the library refuses', function () { A.drawListFilteredDevice(c, [rgba, rgba, rgba], 8, dst, 0); });
bad('drawFilterFactors: too few arguments', function () { A.drawFilterFactors(Int32Array.from([8, 8]), 4, 4); });
bad('drawFilterFactors: sizes a plain array', function () { A.drawFilterFactors([8, 8], 4, 4, 8); });
bad('drawFilterFactors: sizes of three', function () { A.drawFilterFactors(Int32Array.from([8, 8, 8]), 4, 4, 8); });
bad('drawFilterFactors: maxFactor 9', function () { A.drawFilterFactors(Int32Array.from([8, 8]), 4, 4, 9); });
bad('drawFilterFactors: maxFactor 0', function () { A.drawFilterFactors(Int32Array.from([8, 8]), 4, 4, 0); });
bad('drawFilterFactors: canvas width 0', function () { A.drawFilterFactors(Int32Array.from([8, 8]), 0, 4, 8); });
bad('drawFilterFactors: the library refuses', function () { A.drawFilterFactors(Int32Array.from([8, 8, 16385, 8]), 4, 4, 8); });
A.destroy(c);
process.stdout.write(JSON.stringify(out) + '\n');
