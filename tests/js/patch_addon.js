'use strict';
/* The N-API shim's cropPairsTensorDevice / cropSourcesTensorDevice / alignPairsTensorDevice / alignSourcesTensorDevice on the CPU (driven by
 * tests/test_patch_tensor_cpu.py):
 *     node tests/js/patch_addon.js <addon.node built from csrc/ht_napi.cc + tests/js/abi_stub.cc + crop_stub.cc + align_stub.cc + patch_stub.cc>
 * Successful calls (what reaches the C ABI is in the stub's log) and every malformed call (the message each one throws is printed).  One JSON line. */
const A = require(process.argv[2]);
const out = { consts: [A.PATCH_F32, A.PATCH_F16, A.PATCH_BF16, A.PATCH_CHW, A.PATCH_HWC, A.PATCH_RGB, A.PATCH_BGR, A.PATCH_GRAY], thrown: [] };
const FNS = { cropPairs: A.cropPairsTensorDevice, cropSources: A.cropSourcesTensorDevice, alignPairs: A.alignPairsTensorDevice, alignSources: A.alignSourcesTensorDevice };
out.kinds = Object.keys(FNS).map(function (k) { return typeof FNS[k]; });
const c = A.createContext({ cascade: new Uint8Array(64), interval: 5, device: 0 });
A.setGeometry(c, 40, 30, 4, null);
const buf = A.deviceAlloc(c, 100000);
const P = Int32Array.from([7, 3, 256, 0]), PSQ = Int32Array.from([7, 3, 1024, 1]);
const pairs = Int32Array.from([5, 0, 0, 0, 2, 1, 2, 1]);
const rgba = { dev: buf, offset: 50000, width: 7, height: 5, format: A.DRAW_RGBA, matrix: 0, rect: null };
const nv12 = { dev: buf, offset: 51001, width: 23, height: 23, format: A.YUV_NV12, matrix: 1, rect: Int32Array.from([1, 1, 21, 21]) };
const F16 = { dtype: A.PATCH_F16, layout: A.PATCH_CHW, channels: A.PATCH_RGB, scale: Float32Array.from([1 / 255, 2 / 255, 0.5]), bias: Float32Array.from([-1, 0, -0]) };
const F32G = { dtype: A.PATCH_F32, layout: A.PATCH_HWC, channels: A.PATCH_GRAY, scale: Float32Array.from([1, 0, 0]), bias: Float32Array.from([0.25, 0, 0]) };
const BF = { dtype: A.PATCH_BF16, layout: A.PATCH_HWC, channels: A.PATCH_BGR, scale: Float32Array.from([1, 1, 1]), bias: Float32Array.from([0, 0, 0]) };
['crop', 'align'].forEach(function (k) {
  const pairsFn = FNS[k + 'Pairs'], sourcesFn = FNS[k + 'Sources'];
  pairsFn(c, pairs, P, F16, buf, 0);                                          /* the 6-argument form: packed (a patch's 126 bytes rounded up to 4), offset 0, no wait */
  pairsFn(c, pairs.subarray(0, 4), PSQ, F32G, buf, 84 + 16, 8, true);          /* stride, offset, wait */
  sourcesFn(c, Int32Array.from([3, 3]), [rgba, nv12], P, BF, buf, 0);
  sourcesFn(c, Int32Array.from([1, 7]), [nv12, rgba], PSQ, F16, buf, 128 + 4, 12, true);
});
function bad(what, fn) { try { fn(); out.thrown.push([what, null]); } catch (e) { out.thrown.push([what, e.constructor.name + ': ' + e.message]); } }
const small16 = A.deviceAlloc(c, 4 * 128 - 2), small32 = A.deviceAlloc(c, 4 * 252);  /* four f16 patches 128 apart end at 510; four f32 patches are 1008 bytes */
Object.keys(FNS).forEach(function (name) {
  const fn = FNS[name], pairsForm = name.endsWith('Pairs');
  const call = function (fmt, outDev, stride, off, list) {
    if (pairsForm) return fn(c, list || pairs, P, fmt, outDev, stride, off);
    const m = (list || pairs).length >> 1;
    return fn(c, new Int32Array(m), new Array(m).fill(rgba), P, fmt, outDev, stride, off);
  };
  call(F16, small16, 0, 0);                                                    /* exactly fits: the range check uses the tensor's bytes, not w * h * 4 */
  bad(name + ': too few arguments', function () { pairsForm ? fn(c, pairs, P, F16, buf) : fn(c, Int32Array.from([0]), [rgba], P, F16, buf); });
  bad(name + ': no format', function () { pairsForm ? fn(c, pairs, P, buf, 0, 0) : fn(c, Int32Array.from([0]), [rgba], P, buf, 0, 0); });
  bad(name + ': format null', function () { call(null, buf, 0, 0); });
  bad(name + ': format without dtype', function () { call({ layout: 0, channels: 0, scale: F16.scale, bias: F16.bias }, buf, 0, 0); });
  bad(name + ': dtype a string', function () { call(Object.assign({}, F16, { dtype: 'f16' }), buf, 0, 0); });
  bad(name + ': scale a plain array', function () { call(Object.assign({}, F16, { scale: [1, 1, 1] }), buf, 0, 0); });
  bad(name + ': scale a Float64Array', function () { call(Object.assign({}, F16, { scale: Float64Array.from([1, 1, 1]) }), buf, 0, 0); });
  bad(name + ': bias of two', function () { call(Object.assign({}, F16, { bias: Float32Array.from([0, 0]) }), buf, 0, 0); });
  bad(name + ': scale of four', function () { call(Object.assign({}, F16, { scale: Float32Array.from([1, 1, 1, 1]) }), buf, 0, 0); });
  bad(name + ': f16 output two bytes too small', function () { call(F16, A.deviceAlloc(c, 4 * 128 - 4), 0, 0); });
  bad(name + ': f32 output too small for what an RGBA list fits', function () { call(Object.assign({}, F16, { dtype: A.PATCH_F32 }), A.deviceAlloc(c, 4 * 84), 0, 0); });
  bad(name + ': output offset beyond', function () { call(Object.assign({}, F16, { dtype: A.PATCH_F32 }), small32, 0, 4); });
  bad(name + ': out null', function () { call(F16, null, 0, 0); });
  bad(name + ': the library refuses', function () { call(F16, buf, 0, 0, pairs.subarray(0, 6)); });
});
A.destroy(c);
process.stdout.write(JSON.stringify(out) + '\n');
