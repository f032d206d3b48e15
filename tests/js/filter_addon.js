'use strict';
/* The N-API shim's cropPairsFilteredDevice / cropSourcesFilteredDevice / alignPairsFilteredDevice / alignSourcesFilteredDevice /
 * cropFilterFactors / alignFilterFactors on the CPU (driven by tests/test_filter_cpu.py):
 *     node tests/js/filter_addon.js <addon.node built from csrc/ht_napi.cc + tests/js/abi_stub.cc + crop_stub.cc + align_stub.cc + patch_stub.cc + filter_stub.cc>
 * Successful calls (what reaches the C ABI is in the stub's log) and every malformed call (the message each one throws is printed).  One JSON line. */
const A = require(process.argv[2]);
const out = { thrown: [] };
const FNS = { cropPairs: A.cropPairsFilteredDevice, cropSources: A.cropSourcesFilteredDevice, alignPairs: A.alignPairsFilteredDevice, alignSources: A.alignSourcesFilteredDevice };
out.kinds = Object.keys(FNS).map(function (k) { return typeof FNS[k]; }).concat([typeof A.cropFilterFactors, typeof A.alignFilterFactors]);
const c = A.createContext({ cascade: new Uint8Array(64), interval: 5, device: 0 });
A.setGeometry(c, 40, 30, 4, null);
const buf = A.deviceAlloc(c, 100000);
const P = Int32Array.from([7, 3, 256, 0]), PSQ = Int32Array.from([7, 3, 1024, 1]);
const pairs = Int32Array.from([5, 0, 0, 0, 2, 1, 2, 1]);
const rgba = { dev: buf, offset: 50000, width: 7, height: 5, format: A.DRAW_RGBA, matrix: 0, rect: null };
const nv12 = { dev: buf, offset: 51001, width: 23, height: 23, format: A.YUV_NV12, matrix: 1, rect: Int32Array.from([1, 1, 21, 21]) };
const F16 = { dtype: A.PATCH_F16, layout: A.PATCH_CHW, channels: A.PATCH_RGB, scale: Float32Array.from([1 / 255, 2 / 255, 0.5]), bias: Float32Array.from([-1, 0, -0]) };
['crop', 'align'].forEach(function (k) {
  const pairsFn = FNS[k + 'Pairs'], sourcesFn = FNS[k + 'Sources'];
  pairsFn(c, pairs, P, 8, null, buf, 0);                                       /* the 7-argument form: RGBA8, packed, offset 0, no wait */
  pairsFn(c, pairs.subarray(0, 4), PSQ, 1, F16, buf, 128 + 4, 8, true);        /* a format; stride, offset, wait */
  sourcesFn(c, Int32Array.from([3, 3]), [rgba, nv12], P, 3, undefined, buf, 0); /* undefined is null: RGBA8 */
  sourcesFn(c, Int32Array.from([1, 7]), [nv12, rgba], PSQ, 5, F16, buf, 0, 12, true);
});
const rec = Int32Array.from([1, 5, 10, 20, 30, 40, 0, 2, 0, 0, 0, 0]);
out.cropFactors = Array.from(A.cropFilterFactors(rec, 112, 64, 8));
out.cropFactorsKind = A.cropFilterFactors(rec, 112, 64, 8).constructor.name;
out.alignFactors = Array.from(A.alignFilterFactors(Int32Array.from([1, 5, 1024, 0, 0, 2, 0, 0]), Float64Array.from([1, 2, 7 * 65536, 0, 0, -3 * 65536, 0, 0, 0, 0, 0, 0]), 112, 64, 3));
function bad(what, fn) { try { fn(); out.thrown.push([what, null]); } catch (e) { out.thrown.push([what, e.constructor.name + ': ' + e.message]); } }
const small = A.deviceAlloc(c, 4 * 84), small16 = A.deviceAlloc(c, 4 * 128 - 2);  /* four RGBA patches of 7 x 3; four f16 patches 128 apart end at 510 */
Object.keys(FNS).forEach(function (name) {
  const fn = FNS[name], pairsForm = name.endsWith('Pairs');
  const call = function (mf, fmt, outDev, stride, off, list, prm) {
    if (pairsForm) return fn(c, list || pairs, prm || P, mf, fmt, outDev, stride, off);
    const m = (list || pairs).length >> 1;
    return fn(c, new Int32Array(m), new Array(m).fill(rgba), prm || P, mf, fmt, outDev, stride, off);
  };
  call(8, null, small, 0, 0);                                                   /* exactly fits: RGBA8 patches */
  call(8, F16, small16, 0, 0);                                                  /* exactly fits: the tensor's bytes */
  bad(name + ': too few arguments', function () { pairsForm ? fn(c, pairs, P, 8, null, buf) : fn(c, Int32Array.from([0]), [rgba], P, 8, null, buf); });
  bad(name + ': no maxFactor', function () { pairsForm ? fn(c, pairs, P, null, buf, 0, 0) : fn(c, Int32Array.from([0]), [rgba], P, null, buf, 0, 0); });
  bad(name + ': maxFactor a string', function () { call('8', null, buf, 0, 0); });
  bad(name + ': maxFactor 0', function () { call(0, null, buf, 0, 0); });
  bad(name + ': maxFactor 9', function () { call(9, null, buf, 0, 0); });
  bad(name + ': maxFactor -1', function () { call(-1, F16, buf, 0, 0); });
  bad(name + ': format a number', function () { call(8, 16, buf, 0, 0); });
  bad(name + ': format without dtype', function () { call(8, { layout: 0, channels: 0, scale: F16.scale, bias: F16.bias }, buf, 0, 0); });
  bad(name + ': scale a plain array', function () { call(8, Object.assign({}, F16, { scale: [1, 1, 1] }), buf, 0, 0); });
  bad(name + ': width 0', function () { call(8, null, buf, 0, 0, null, Int32Array.from([0, 3, 256, 0])); });
  bad(name + ': height 1025', function () { call(8, null, buf, 0, 0, null, Int32Array.from([7, 1025, 256, 0])); });
  bad(name + ': params of three', function () { call(8, null, buf, 0, 0, null, Int32Array.from([7, 3, 256])); });
  bad(name + ': RGBA output four bytes too small', function () { call(8, null, A.deviceAlloc(c, 4 * 84 - 4), 0, 0); });
  bad(name + ': f16 output two bytes too small', function () { call(8, F16, A.deviceAlloc(c, 4 * 128 - 4), 0, 0); });
  bad(name + ': f16 output where only RGBA fits', function () { call(8, F16, small, 0, 0); });
  bad(name + ': output offset beyond', function () { call(8, null, small, 0, 4); });
  bad(name + ': out null', function () { call(8, null, null, 0, 0); });
  bad(name + ': the library refuses', function () { call(8, null, buf, 0, 0, pairs.subarray(0, 6)); });
});
bad('cropFilterFactors: too few arguments', function () { A.cropFilterFactors(rec, 112, 64); });
bad('cropFilterFactors: records a plain array', function () { A.cropFilterFactors([1, 5, 10, 20, 30, 40], 112, 64, 8); });
bad('cropFilterFactors: records of five', function () { A.cropFilterFactors(rec.subarray(0, 5), 112, 64, 8); });
bad('cropFilterFactors: maxFactor 9', function () { A.cropFilterFactors(rec, 112, 64, 9); });
bad('cropFilterFactors: width 0', function () { A.cropFilterFactors(rec, 0, 64, 8); });
bad('alignFilterFactors: terms missing', function () { A.alignFilterFactors(Int32Array.from([1, 5, 1024, 0]), 112, 64, 8, 1); });
bad('alignFilterFactors: terms of five', function () { A.alignFilterFactors(Int32Array.from([1, 5, 1024, 0]), new Float64Array(5), 112, 64, 8); });
bad('alignFilterFactors: height 1025', function () { A.alignFilterFactors(Int32Array.from([1, 5, 1024, 0]), new Float64Array(6), 112, 1025, 8); });
A.destroy(c);
process.stdout.write(JSON.stringify(out) + '\n');
