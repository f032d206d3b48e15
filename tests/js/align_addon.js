'use strict';
/* The N-API shim's alignPairsDevice / alignSourcesDevice / alignResult on the CPU (driven by tests/test_align_cpu.py):
 *     node tests/js/align_addon.js <addon.node built from csrc/ht_napi.cc + tests/js/abi_stub.cc + tests/js/crop_stub.cc + tests/js/align_stub.cc>
 * Successful calls (what reaches the C ABI is in the stub's log) and every malformed call (the message each one throws is printed).
 * ONE device buffer holds the sources and the patches, so that the stub can log plane pointers relative to the output.  One JSON line. */
const A = require(process.argv[2]);
const out = { consts: [A.ALIGN_EMPTY, A.ALIGN_FACE, A.ALIGN_SQUARE, typeof A.alignPairsDevice, typeof A.alignSourcesDevice, typeof A.alignResult], thrown: [] };
const c = A.createContext({ cascade: new Uint8Array(64), interval: 5, device: 0 });
A.setGeometry(c, 40, 30, 4, null);
const pb = 7 * 3 * 4;
const buf = A.deviceAlloc(c, 100000), small = A.deviceAlloc(c, 4 * pb);
const P = Int32Array.from([7, 3, 256, 0]), PSQ = Int32Array.from([7, 3, 1024, A.ALIGN_SQUARE]);
const pairs = Int32Array.from([5, 0, 0, 0, 2, 1, 2, 1]);
const rgba = { dev: buf, offset: 50000, width: 7, height: 5, format: A.DRAW_RGBA, matrix: 0, rect: null };
const nv12 = { dev: buf, offset: 51001, width: 23, height: 23, format: A.YUV_NV12, matrix: 1, rect: Int32Array.from([1, 1, 21, 21]) };
const i420 = { dev: buf, offset: 54000, width: 97, height: 81, format: A.YUV_I420, matrix: 3 };
A.alignPairsDevice(c, pairs, P, buf, 0);                                           /* the 5-argument form: packed patches at offset 0, no wait */
A.alignPairsDevice(c, pairs.subarray(0, 4), PSQ, buf, pb + 16, 8, true);           /* stride, offset, wait */
A.alignSourcesDevice(c, Int32Array.from([3, 3]), [rgba, nv12], P, buf, 0);
A.alignSourcesDevice(c, Int32Array.from([1, 0, 7, 7]), [i420, nv12, rgba, rgba], PSQ, buf, pb + 4, 12, true);
const r = A.alignResult(c, 4);
out.result = { records: Array.from(r.records), terms: Array.from(r.terms), kinds: [r.records.constructor.name, r.terms.constructor.name] };
function bad(what, fn) { try { fn(); out.thrown.push([what, null]); } catch (e) { out.thrown.push([what, e.constructor.name + ': ' + e.message]); } }
bad('pairs: too few arguments', function () { A.alignPairsDevice(c, pairs, P, buf); });
bad('pairs: no context', function () { A.alignPairsDevice(buf, pairs, P, buf, 0); });
bad('pairs: a plain array', function () { A.alignPairsDevice(c, [5, 0], P, buf, 0); });
bad('pairs: odd length', function () { A.alignPairsDevice(c, Int32Array.from([5, 0, 1]), P, buf, 0); });
bad('pairs: none', function () { A.alignPairsDevice(c, new Int32Array(0), P, buf, 0); });
bad('pairs: 65536', function () { A.alignPairsDevice(c, new Int32Array(2 * 65536), Int32Array.from([1, 1, 256, 0]), A.deviceAlloc(c, 4 * 65536), 0); });
bad('pairs: params of three', function () { A.alignPairsDevice(c, pairs, Int32Array.from([7, 3, 256]), buf, 0); });
bad('pairs: params of five', function () { A.alignPairsDevice(c, pairs, Int32Array.from([7, 3, 256, 0, 0]), buf, 0); });
bad('pairs: params a Float64Array', function () { A.alignPairsDevice(c, pairs, Float64Array.from([7, 3, 256, 0]), buf, 0); });
bad('pairs: width 0', function () { A.alignPairsDevice(c, pairs, Int32Array.from([0, 3, 256, 0]), buf, 0); });
bad('pairs: height 1025', function () { A.alignPairsDevice(c, pairs, Int32Array.from([7, 1025, 256, 0]), buf, 0); });
bad('pairs: out null', function () { A.alignPairsDevice(c, pairs, P, null, 0); });
bad('pairs: out a context', function () { A.alignPairsDevice(c, pairs, P, c, 0); });
bad('pairs: stride a string', function () { A.alignPairsDevice(c, pairs, P, buf, 'packed'); });
bad('pairs: negative offset', function () { A.alignPairsDevice(c, pairs, P, buf, 0, -4); });
bad('pairs: output too small', function () { A.alignPairsDevice(c, Int32Array.from([0, 0, 1, 0, 2, 0, 3, 0, 4, 0]), P, small, 0); });
bad('pairs: output offset beyond', function () { A.alignPairsDevice(c, pairs, P, small, 0, 4); });
bad('pairs: output stride beyond', function () { A.alignPairsDevice(c, pairs.subarray(0, 4), P, small, 4 * pb); });
bad('pairs: the library refuses', function () { A.alignPairsDevice(c, pairs.subarray(0, 6), P, buf, 0); });
bad('sources: too few arguments', function () { A.alignSourcesDevice(c, Int32Array.from([0]), [rgba], P, buf); });
bad('sources: streams a plain array', function () { A.alignSourcesDevice(c, [0], [rgba], P, buf, 0); });
bad('sources: entries no array', function () { A.alignSourcesDevice(c, Int32Array.from([0]), rgba, P, buf, 0); });
bad('sources: no entries', function () { A.alignSourcesDevice(c, new Int32Array(0), [], P, buf, 0); });
bad('sources: one stream for two entries', function () { A.alignSourcesDevice(c, Int32Array.from([0]), [rgba, nv12], P, buf, 0); });
bad('sources: entry no object', function () { A.alignSourcesDevice(c, Int32Array.from([0, 1]), [rgba, 5], P, buf, 0); });
bad('sources: entry without dev', function () { A.alignSourcesDevice(c, Int32Array.from([0]), [{ width: 7, height: 5, format: A.DRAW_RGBA }], P, buf, 0); });
bad('sources: frame beyond its buffer', function () { A.alignSourcesDevice(c, Int32Array.from([0]), [Object.assign({}, rgba, { offset: 100000 - 100 })], P, buf, 0); });
bad('sources: rect a plain array', function () { A.alignSourcesDevice(c, Int32Array.from([0]), [Object.assign({}, rgba, { rect: [0, 0, 4, 4] })], P, buf, 0); });
bad('sources: width 1025', function () { A.alignSourcesDevice(c, Int32Array.from([0]), [rgba], Int32Array.from([1025, 3, 256, 0]), buf, 0); });
bad('sources: output too small', function () { A.alignSourcesDevice(c, Int32Array.from([0, 0, 0, 0, 0]), [rgba, rgba, rgba, rgba, rgba], P, small, 0); });
bad('sources: out null', function () { A.alignSourcesDevice(c, Int32Array.from([0]), [rgba], P, undefined, 0); });
bad('sources: the library refuses', function () { A.alignSourcesDevice(c, Int32Array.from([0, 1, 2]), [rgba, rgba, rgba], P, buf, 0); });
bad('result: too few arguments', function () { A.alignResult(c); });
bad('result: n 0', function () { A.alignResult(c, 0); });
bad('result: n a string', function () { A.alignResult(c, 'four'); });
bad('result: the library refuses', function () { A.alignResult(c, 5); });
A.destroy(c);
process.stdout.write(JSON.stringify(out) + '\n');
